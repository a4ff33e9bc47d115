"""Host-side bindings of the C ABI (include/gdkvm.h) for torch tensors.

Every function checks shapes on the host, hands raw device pointers + the current HIP stream to
libgdkvm_hip.so and returns torch tensors.  No fallback path exists: a missing library or a CPU tensor
raises (the product must never silently run anything but the HIP kernels).

The rule of this module: ONE helper launches (_call: device, symbol, C arguments, stream, error under the name of the entry that
ran), ONE sizes workspaces (_bytes, with _workspace / _grown_workspace allocating from it); a wrapper checks shapes, allocates its
outputs and names its entry point once.  Pointers are never taken by hand: tensors go to _call as they are, workspaces as _Ws(t).
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import os
from typing import Optional, Tuple

import torch

RULE_GATED_LINEAR, RULE_DELTA_PARALLEL, RULE_DELTA_SEQUENTIAL = 0, 1, 2
FLAG_NORMALIZE_QK, FLAG_GATE_LOGITS, FLAG_TRAIN, FLAG_WIDE_RANGE = 1, 2, 4, 8


def recurrence_flags(rule: int, flags: int) -> int:
    """Flags for the split prep / apply / transition entry points: rule delta_parallel is not contractive, so its state
    recurrence runs on the full-range three-term operands (gdkvm_scan_fwd adds the flag itself)."""
    return flags | FLAG_WIDE_RANGE if rule == RULE_DELTA_PARALLEL else flags
F32, BF16 = 0, 1

_PKG = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_PKG, "libgdkvm_hip.so")
_lib = None
_vp, _sz, _i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int

# symbol -> (restype, argtypes): must list every entry point include/gdkvm.h declares
SIGNATURES = {
    "gdkvm_abi_version": (_i, []),
    "gdkvm_last_error": (ctypes.c_char_p, []),
    "gdkvm_scan_workspace_bytes": (_sz, [_i] * 6),
    "gdkvm_scan_fwd": (_i, [_vp] * 10 + [_sz] + [_i] * 9 + [_vp]),
    "gdkvm_scan_prep": (_i, [_vp] * 5 + [_sz] + [_i] * 9 + [_vp]),
    "gdkvm_scan_apply": (_i, [_vp] * 7 + [_sz] + [_i] * 8 + [_vp]),
    "gdkvm_scan_prep_normed": (_i, [_vp] * 6 + [_sz] + [_i] * 9 + [_vp]),
    "gdkvm_scan_fwd_normed": (_i, [_vp] * 10 + [_sz] + [_i] * 9 + [_vp]),
    "gdkvm_scan_transition": (_i, [_vp] * 4 + [_sz] + [_i] * 8 + [_vp]),
    "gdkvm_scan_stitch": (_i, [_vp] * 5 + [_i] * 5 + [_vp]),
    "gdkvm_scan_status": (_i, [_vp, _sz] + [_i] * 7 + [_vp]),
    "gdkvm_scan_bwd_workspace_bytes": (_sz, [_i] * 6),
    "gdkvm_scan_state_bwd": (_i, [_vp] * 6 + [_sz] + [_vp] * 8 + [_sz] + [_i] * 9 + [_vp]),
    "gdkvm_scan_bwd": (_i, [_vp] * 7 + [_sz] + [_vp] * 9 + [_sz] + [_i] * 9 + [_vp]),
    "gdkvm_scan_segments": (_i, [_i] * 5),
    "gdkvm_scan_segmented_workspace_bytes": (_sz, [_i] * 7),
    "gdkvm_scan_fwd_segmented": (_i, [_vp] * 9 + [_sz] + [_i] * 10 + [_vp]),
    "gdkvm_scan_normalizer_workspace_bytes": (_sz, [_i] * 7),
    "gdkvm_scan_fwd_normalizer": (_i, [_vp] * 11 + [_sz] + [_i] * 9 + [ctypes.c_float, _vp]),
    "gdkvm_lkva_read": (_i, [_vp] * 4 + [_i] * 7 + [_vp]),
    "gdkvm_mask_embed_add": (_i, [_vp] * 3 + [_i] * 7 + [_vp]),
    "gdkvm_mask_embed_wgrad_workspace_bytes": (_sz, [_i] * 4),
    "gdkvm_mask_embed_wgrad": (_i, [_vp] * 4 + [_sz] + [_i] * 7 + [_vp]),
    "gdkvm_scan_train_workspace_bytes": (_sz, [_i] * 7),
    "gdkvm_scan_train_fwd": (_i, [_vp] * 9 + [_sz] + [_i] * 9 + [_vp]),
    "gdkvm_scan_train_bwd": (_i, [_vp] * 14 + [_sz] + [_i] * 9 + [_vp]),
    "gdkvm_readout_fwd": (_i, [_vp] * 3 + [_i] * 9 + [_vp]),
    "gdkvm_readout_bwd": (_i, [_vp] * 5 + [_i] * 9 + [_vp]),
    "gdkvm_gemm_nt": (_i, [_vp] * 4 + [_i] * 4 + [_vp]),
    "gdkvm_gemm_tn_workspace_bytes": (_sz, [_i] * 3),
    "gdkvm_gemm_tn": (_i, [_vp] * 4 + [_sz] + [_i] * 4 + [_vp]),
    "gdkvm_gemm_tn_colsum_workspace_bytes": (_sz, [_i] * 3),
    "gdkvm_gemm_tn_colsum": (_i, [_vp] * 5 + [_sz] + [_i] * 4 + [_vp]),
    "gdkvm_kpff_workspace_bytes": (_sz, [_i] * 4),
    "gdkvm_kpff_fwd": (_i, [_vp] * 9 + [_sz] + [_i] * 7 + [_vp]),
    "gdkvm_kpff_fwd_packed": (_i, [_vp] * 9 + [_sz] + [_i] * 7 + [_vp]),
    "gdkvm_kpff_fwd_train": (_i, [_vp] * 13 + [_sz] + [_i] * 7 + [_vp]),
    "gdkvm_kpff_bwd_pre": (_i, [_vp] * 7 + [_i] * 4 + [_vp]),
    "gdkvm_kpff_bwd_post": (_i, [_vp] * 7 + [_i] * 7 + [_vp]),
    "gdkvm_argmax_dice": (_i, [_vp] * 4 + [_i] * 5 + [_vp]),
    "gdkvm_bias_act": (_i, [_vp] * 4 + [_sz] + [_i] * 3 + [_vp]),
    "gdkvm_head_logits": (_i, [_vp] * 4 + [_i] * 6 + [_vp]),
    "gdkvm_head_bwd_workspace_bytes": (_sz, [_i] * 2),
    "gdkvm_head_bwd": (_i, [_vp] * 7 + [_sz] + [_i] * 6 + [_vp]),
    "gdkvm_proj_rows": (_i, [_vp] * 6 + [ctypes.c_longlong] + [_i] * 5 + [_vp]),
    "gdkvm_stem_conv_pool": (_i, [_vp] * 4 + [_i] * 4 + [_vp]),
    "gdkvm_stem_conv_pool_nchw": (_i, [_vp] * 4 + [_i] * 5 + [_vp]),
    "gdkvm_stem_conv_nchw": (_i, [_vp] * 3 + [_i] * 5 + [_vp]),
    "gdkvm_stem_pack_s2d": (_i, [_vp, _vp, _i] + [ctypes.c_longlong] * 4 + [_vp]),
    "gdkvm_stem_wgrad_workspace_bytes": (_sz, [_i] * 3),
    "gdkvm_stem_wgrad_nchw": (_i, [_vp] * 3 + [ctypes.c_longlong] * 4 + [_vp, _sz] + [_i] * 5 + [_vp]),
    "gdkvm_gate_logits": (_i, [_vp] * 7 + [_i] * 5 + [_vp]),
    "gdkvm_proj_gates": (_i, [_vp] * 13 + [_i] * 7 + [_vp]),
    "gdkvm_conv_bias_act": (_i, [_vp] * 5 + [_i] * 12 + [_vp]),
    "gdkvm_conv3x3_pack_weights": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "gdkvm_conv_igemm_pack_weights": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "gdkvm_conv_down_bias_act": (_i, [_vp] * 4 + [_i] + [_vp] * 3 + [_i] * 10 + [_vp]),
    "gdkvm_conv_cat_bias_act": (_i, [_vp] * 6 + [_i] * 9 + [_vp]),
    "gdkvm_conv_upcat_bias_act": (_i, [_vp] * 6 + [_i] * 9 + [_vp]),
    "gdkvm_conv_s2_dgrad_pack_bytes": (_sz, [_i] * 3),
    "gdkvm_conv_s2_pack_train": (_i, [_vp] * 7 + [_i, _i, _vp]),
    "gdkvm_conv_s2_dgrad": (_i, [_vp] * 4 + [_i] * 7 + [_vp]),
    "gdkvm_conv_wgrad_strided_workspace_bytes": (_sz, [_i] * 9),
    "gdkvm_conv_wgrad_strided": (_i, [_vp] * 3 + [ctypes.c_longlong] * 4 + [_vp, _sz] + [_i] * 10 + [_vp]),
    "gdkvm_conv3x3_pack_weights_dgrad": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "gdkvm_conv3x3_pack_weights_train": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gdkvm_conv3x3_wgrad_workspace_bytes": (_sz, [_i] * 5),
    "gdkvm_conv3x3_wgrad": (_i, [_vp, _vp, _vp, _vp, _sz] + [_i] * 6 + [_vp]),
    "gdkvm_conv3x3_wgrad_krsc": (_i, [_vp, _vp, _vp, _vp, _sz] + [_i] * 6 + [_vp]),
    "gdkvm_upsample_cat": (_i, [_vp] * 3 + [_i] * 8 + [_vp]),
    "gdkvm_upsample_cat_bwd": (_i, [_vp] * 3 + [_i] * 8 + [_vp]),
    "gdkvm_bias_relu_maxpool": (_i, [_vp] * 3 + [_i] * 7 + [_vp]),
    "gdkvm_stem_s2d": (_i, [_vp] * 2 + [_i] * 6 + [_vp]),
    "gdkvm_upsample_argmax_dice": (_i, [_vp] * 4 + [_i] * 7 + [_vp]),
    "gdkvm_head_upsample_argmax_dice": (_i, [_vp] * 6 + [_i] * 8 + [_vp]),
    "gdkvm_maxpool_fwd": (_i, [_vp] * 3 + [_i] * 5 + [_vp]),
    "gdkvm_maxpool_bwd": (_i, [_vp] * 3 + [_i] * 5 + [_vp]),
    "gdkvm_seg_loss_workspace_bytes": (_sz, [_i]),
    "gdkvm_seg_loss_fwd": (_i, [_vp] * 4 + [_sz] + [_i] * 6 + [ctypes.c_float] * 2 + [_i, _i, _vp]),
    "gdkvm_seg_loss_bwd": (_i, [_vp] * 3 + [_sz] + [_vp] * 2 + [_i] * 8 + [_vp]),
    "gdkvm_seg_loss_boundary_workspace_bytes": (_sz, [_i]),
    "gdkvm_seg_loss_boundary_fwd": (_i, [_vp] * 5 + [_sz] + [_i] * 6 + [ctypes.c_float] * 3 + [ctypes.c_uint, _i, _i, _vp]),
    "gdkvm_seg_loss_boundary_bwd": (_i, [_vp] * 4 + [_sz] + [_vp] * 2 + [_i] * 6 + [ctypes.c_uint, _i, _i, _vp]),
    "gdkvm_bn_workspace_bytes": (_sz, [_i]),
    "gdkvm_bn_fwd_train": (_i, [_vp] * 9 + [_sz, ctypes.c_longlong, _i, ctypes.c_float, ctypes.c_float, _i, _i, _vp]),
    "gdkvm_bn_bwd": (_i, [_vp] * 10 + [_sz, ctypes.c_longlong, _i, _i, _i, _vp]),
    "gdkvm_bn_pool_fwd_train": (_i, [_vp] * 9 + [_sz] + [_i] * 4 + [ctypes.c_float] * 2 + [_i, _vp]),
    "gdkvm_bn_pool_bwd": (_i, [_vp] * 9 + [_sz] + [_i] * 5 + [_vp]),
    "gdkvm_augment_clips": (_i, [_vp] * 5 + [_i] * 8 + [_vp]),
    "gdkvm_lv_measure": (_i, [_vp] * 4 + [_i] * 5 + [_vp]),
    "gdkvm_lv_measure_mm": (_i, [_vp] * 5 + [_i] * 5 + [_vp]),
    "gdkvm_lv_ef": (_i, [_vp] * 6 + [_i, _i, ctypes.c_int64, _vp]),
    "gdkvm_lv_beats": (_i, [_vp] * 7 + [_i] * 5 + [ctypes.c_int64, _vp]),
    "gdkvm_lv_biplane": (_i, [_vp] * 7 + [_i] * 4 + [_vp]),
    "gdkvm_lv_contour": (_i, [_vp] * 3 + [_i] * 4 + [ctypes.c_uint] * 2 + [_vp]),
    "gdkvm_largest_component_workspace_bytes": (_sz, [_i] * 3),
    "gdkvm_largest_component": (_i, [_vp] * 5 + [_sz] + [_i] * 6 + [_vp]),
    "gdkvm_fill_holes_workspace_bytes": (_sz, [_i] * 3),
    "gdkvm_fill_holes": (_i, [_vp] * 5 + [_sz] + [_i] * 6 + [_vp]),
    "gdkvm_temporal_vote_workspace_bytes": (_sz, [_i] * 5),
    "gdkvm_temporal_vote": (_i, [_vp] * 6 + [_sz] + [_i] * 6 + [_vp]),
    "gdkvm_mask_to_native_workspace_bytes": (_sz, [_i] * 5),
    "gdkvm_mask_to_native": (_i, [_vp] * 5 + [_sz, _vp, _sz] + [_i] * 5 + [_vp]),
    "gdkvm_frames_from_native_workspace_bytes": (_sz, [_i] * 6),
    "gdkvm_frames_from_native": (_i, [_vp] * 3 + [_sz, _vp, _sz] + [_i] * 6 + [_vp]),
    "gdkvm_overlay_native_workspace_bytes": (_sz, [_i] * 4),
    "gdkvm_overlay_native": (_i, [_vp] * 7 + [_sz, _vp, _sz] + [_i] * 5 + [_vp]),
    "gdkvm_surface_distance_workspace_bytes": (_sz, [_i] * 3),
    "gdkvm_surface_distance": (_i, [_vp] * 4 + [_sz] + [_i] * 4 + [_vp]),
    "gdkvm_surface_distance_mm_workspace_bytes": (_sz, [_i] * 3),
    "gdkvm_surface_distance_mm": (_i, [_vp] * 5 + [_sz] + [_i] * 4 + [_vp]),
    "gdkvm_surface_distance_native_workspace_bytes": (_sz, [_i, _i, ctypes.c_longlong, ctypes.c_longlong]),
    "gdkvm_surface_distance_native": (_i, [_vp] * 5 + [_sz, _vp, _sz] + [_i] * 3 + [_vp]),
    "gdkvm_lv_measure_native": (_i, [_vp] * 7 + [_sz, ctypes.c_longlong] + [_i] * 4 + [_vp]),
    "gdkvm_signed_distance_workspace_bytes": (_sz, [_i] * 4),
    "gdkvm_signed_distance": (_i, [_vp] * 3 + [_sz] + [_i] * 4 + [ctypes.c_uint, _vp]),
    "gdkvm_adamw_workspace_bytes": (_sz, [_i, ctypes.c_longlong]),
    "gdkvm_adamw_step": (_i, [_vp] * 7 + [_i, _vp, _vp, _sz] + [ctypes.c_double] * 8 + [ctypes.c_longlong] * 2 + [_i, _vp]),
}


class GdkvmError(RuntimeError):
    pass


def library_path() -> str:
    return _SO


def load():
    """dlopen libgdkvm_hip.so and bind every ABI symbol.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise GdkvmError(f"{_SO} not found: build it with `python -m gdkvm_amd.build` "
                             "(there is no fallback path)")
        lib = ctypes.CDLL(_SO)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        if lib.gdkvm_abi_version() != 1:
            raise GdkvmError(f"ABI version mismatch: {lib.gdkvm_abi_version()}")
        _lib = lib
    return _lib


def require_native():
    """Fail loudly unless the HIP library is loaded and a GPU is present."""
    load()
    if not torch.cuda.is_available():
        raise GdkvmError("no HIP device visible: the GDKVM ops have no CPU path")


def _check(rc: int, what: str):
    if rc != 0:
        raise GdkvmError(f"{what} failed ({rc}): {load().gdkvm_last_error().decode()}")


def _io_dtype(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise GdkvmError(f"unsupported io dtype {t.dtype} (float32 or bfloat16)")


def _dev(*ts):
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise GdkvmError("GDKVM ops need device tensors (no CPU path)")
        if not t.is_contiguous():
            raise GdkvmError("GDKVM ops need contiguous tensors")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise GdkvmError("tensors on different devices")
    return dev


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


class _Ws:
    """Marks a tensor as a workspace argument of _call: it becomes (pointer, size in BYTES); _Ws(None) is (NULL, 0)."""
    __slots__ = ("t",)

    def __init__(self, t: Optional[torch.Tensor]):
        self.t = t


def _c_args(args) -> list:
    """The C values of a wrapper's arguments (pure: no device needed): a tensor is its pointer, None and an empty tensor are NULL (_ptr),
    a _Ws is pointer and byte count, everything else (ints, floats, ctypes values) passes through.  Runs once per launch, for ~20
    arguments: ints leave on the first test, and an empty tensor's data_ptr() is 0, which `or None` turns into what _ptr returns."""
    out = []
    add = out.append
    for a in args:
        if type(a) is int:
            add(a)
        elif isinstance(a, torch.Tensor):
            add(a.data_ptr() or None)
        elif type(a) is _Ws:
            out += (None, 0) if a.t is None else (a.t.data_ptr() or None, a.t.nbytes)
        else:
            add(a)
    return out


_BOUND = {}


def _call(name: str, dev, *args) -> None:
    """THE launch: entry point `name` (looked up once) with `dev` current, on dev's current stream (appended as the last argument).  Raises
    GdkvmError naming `name` with the library's own message."""
    fn = _BOUND.get(name)
    if fn is None:
        fn = _BOUND[name] = getattr(load(), name)
    with torch.cuda.device(dev):
        rc = fn(*_c_args(args), _stream(dev))
    if rc:
        _check(rc, name)


_SIZES = {}


def _bytes(name: str, dev, *dims) -> int:
    """Size query `name`(*dims), asked once per (entry, device, dims) with `dev` current (some sizes depend on the device's CU count; dev
    None: whichever is current) and remembered: a size is a pure function of these."""
    n = _SIZES.get((name, dev, dims))
    if n is None:
        with torch.cuda.device(dev) if dev is not None else contextlib.nullcontext():
            n = _SIZES[(name, dev, dims)] = int(getattr(load(), name)(*dims))
    return n


def _workspace(name: str, dev, *dims, floor: int = 0) -> torch.Tensor:
    """A fresh uint8 workspace of the size the `*_workspace_bytes` entry `name` asks for (at least `floor` bytes)."""
    return torch.empty(max(floor, _bytes(name, dev, *dims)), dtype=torch.uint8, device=dev)


_GROWN_WS = {}


def _grown_workspace(name: str, dev, *dims) -> torch.Tensor:
    """One workspace per (size entry, device, stream), grown to the largest request and never shrunk: calls on a stream are ordered,
    so the next layer may overwrite it.  Different size entries never share a buffer."""
    need = max(16, _bytes(name, dev, *dims))
    key = (name, dev, _stream(dev))
    ws = _GROWN_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _GROWN_WS[key] = torch.empty(need, dtype=torch.uint8, device=dev)
    return ws


def _channels_last(what: str, *ts, dtype=None, shape: str = "[N,C,H,W]") -> None:
    for t in ts:
        if t.dim() != 4 or not t.is_cuda or (dtype is not None and t.dtype != dtype) or not t.is_contiguous(memory_format=torch.channels_last):
            raise GdkvmError(f"{what} needs channels_last{'' if dtype is None else ' ' + str(dtype)[6:]} {shape} device tensors (no CPU path)")


def _u8_target(target: Optional[torch.Tensor], BT: int, H: int, W: int) -> None:
    if target is not None and (target.dtype != torch.uint8 or tuple(target.shape) != (BT, H, W)):
        raise GdkvmError("target must be uint8 [BT,H,W]")


def _mask_frames(what: str, mask: torch.Tensor, cls: int, **same):
    """The per-frame mask kernels' common checks: mask uint8 [..., H, W] with sides in 1..LV_MAX_SIDE, cls in 0..254, and every tensor of
    `same` (name=tensor; None passes) of mask's dtype and shape.  Returns (lead, frames, H, W): the leading shape and its product."""
    if mask.dtype != torch.uint8 or mask.dim() < 2:
        raise GdkvmError(f"{what}: mask must be uint8 [..., H, W], got {mask.dtype} {tuple(mask.shape)}")
    H, W = mask.shape[-2:]
    if not (1 <= H <= LV_MAX_SIDE and 1 <= W <= LV_MAX_SIDE):
        raise GdkvmError(f"{what}: H = {H}, W = {W} outside 1..{LV_MAX_SIDE}")
    if not 0 <= int(cls) <= 254:
        raise GdkvmError(f"{what}: cls = {cls} outside 0..254")
    for name, t in same.items():
        if t is not None and (t.dtype != torch.uint8 or tuple(t.shape) != tuple(mask.shape)):
            raise GdkvmError(f"{what}: {name} must be uint8 {tuple(mask.shape)}, got {t.dtype} {tuple(t.shape)}")
    lead = tuple(mask.shape[:-2])
    return lead, math.prod(lead), H, W


def _f32_vectors(what: str, c: int, *ts) -> None:
    for t in ts:
        if t is not None and (t.dtype != torch.float32 or t.numel() != c or not t.is_contiguous()):
            raise GdkvmError(f"{what}: weight / bias / running statistics must be contiguous float32 [C]")


def _scan_operands(q, k, v, alpha, beta, state):
    """The shape / dtype contract every scan entry shares; returns (B, T, N, Hh, Dk, Dv)."""
    if q.dim() != 5 or k.shape != q.shape or v.dim() != 5 or v.shape[:4] != q.shape[:4]:
        raise GdkvmError(f"bad shapes q{tuple(q.shape)} k{tuple(k.shape)} v{tuple(v.shape)}")
    B, T, N, Hh, Dk = q.shape
    Dv = v.shape[-1]
    if tuple(alpha.shape) != (B, T, Hh) or tuple(beta.shape) != (B, T, N, Hh):
        raise GdkvmError(f"bad gate shapes alpha{tuple(alpha.shape)} beta{tuple(beta.shape)}")
    if k.dtype != q.dtype or v.dtype != q.dtype:
        raise GdkvmError("q, k, v must share one dtype")
    if alpha.dtype != torch.float32 or beta.dtype != torch.float32:
        raise GdkvmError("alpha / beta must be float32")
    if state is not None and (tuple(state.shape) != (B, Hh, Dk, Dv) or state.dtype != torch.float32):
        raise GdkvmError("state must be float32 [B,Hh,Dk,Dv]")
    return B, T, N, Hh, Dk, Dv


KERNEL_DK = 64                # per-head key dim the fast kernels are built for (include/gdkvm.h; narrower keys run on them through zero
                              # channels, wider ones -- up to 256 -- on the general kernel of csrc/gdr_general.hip, trained through gdr_general_bwd.hip)


def _pad_keys(q, k, state):
    """Key dims below 64 run on the Dk = 64 kernels with zero channels appended: norms, Gram matrices and read-outs are
    unchanged, P stays the identity on the extra rows and a zero extra block of the state stays zero -- the result on the real
    rows is exactly that of the narrower problem (tests/test_scan_gpu.py).  Layout plumbing only; nothing is computed here."""
    pad = KERNEL_DK - q.shape[-1]
    Fn = torch.nn.functional
    return Fn.pad(q, (0, pad)), Fn.pad(k, (0, pad)), (None if state is None else Fn.pad(state, (0, 0, 0, pad)))


def scan_workspace_bytes(B, T, Hh, N, Dk, Dv) -> int:
    return _bytes("gdkvm_scan_workspace_bytes", None, B, T, Hh, N, Dk, Dv)


def scan_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, alpha: torch.Tensor, beta: torch.Tensor,
             state: Optional[torch.Tensor] = None, rule: int = RULE_DELTA_SEQUENTIAL, flags: int = 0,
             workspace: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
             state_out: Optional[torch.Tensor] = None, state_hist: Optional[torch.Tensor] = None,
             readout: bool = True, norms: Optional[torch.Tensor] = None, check: bool = False) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
    """Fused LKVA read + GDR write over T frames (gdkvm_scan_fwd).

    q,k [B,T,N,Hh,Dk]  v [B,T,N,Hh,Dv]  (f32|bf16)   alpha [B,T,Hh]  beta [B,T,N,Hh]  state [B,Hh,Dk,Dv] (f32)
    returns (R [B,T,N,Hh,Dv] in the io dtype, S_T [B,Hh,Dk,Dv] f32).
    Range: the default recurrence carries the state as fp16 pairs at 2^-e with e sized from the call's own bound on the state
    (include/gdkvm.h, GDKVM_FLAG_WIDE_RANGE), so values and carried states of any magnitude are served for rules 0 and 2 (with unit-norm keys and gates in [0, 1]: flags=3, or inputs the caller normalised); the
    one refusal -- frames of more than 64 tokens with values ~1e5x the usual -- returns NaNs, and FLAG_WIDE_RANGE serves it.
    check=True: wait for the call and raise GdkvmError if the data left that range (gdkvm_scan_status; synchronises the stream).
    norms [B*T*N, Hh, 2] fp32 (ops.proj_gates): the inverse key / query norms came with the projections (gdkvm_scan_fwd_normed:
    the frame-parallel kernel neither reads q nor reduces anything in its first phase); needs FLAG_NORMALIZE_QK, Dk = 64."""
    B, T, N, Hh, Dk, Dv = _scan_operands(q, k, v, alpha, beta, state)
    if q.shape[-1] < KERNEL_DK and state_hist is None and q.shape[-1] % 8:      # key widths that are no multiple of 8: padded here
        qp, kp, sp = _pad_keys(q, k, state)                # (multiples of 8 below 64: gdkvm_scan_fwd zero-extends them itself)
        r, s = scan_fwd(qp, kp, v, alpha, beta, sp, rule, flags, workspace, out, None, None, readout, None, check)
        s = s[:, :, :q.shape[-1]].contiguous()
        if state_out is not None:
            state_out.copy_(s)
            s = state_out
        return r, s
    dev = _dev(q, k, v, alpha, beta, state, workspace, out, state_out, state_hist)
    io = _io_dtype(q)
    if workspace is None:
        workspace = _workspace("gdkvm_scan_workspace_bytes", dev, B, T, Hh, N, Dk, Dv)
    r = None if not readout else (out if out is not None else torch.empty((B, T, N, Hh, Dv), dtype=q.dtype, device=dev))
    s = state_out if state_out is not None else torch.empty((B, Hh, Dk, Dv), dtype=torch.float32, device=dev)
    if norms is not None:
        if state_hist is not None or norms.dtype != torch.float32 or norms.numel() != B * T * N * Hh * 2 or not norms.is_contiguous() \
                or norms.device != dev:
            raise GdkvmError("scan_fwd: norms must be contiguous float32 [B*T*N, Hh, 2] on the inputs' device (inference: no state_hist)")
        name, extra = "gdkvm_scan_fwd_normed", (norms, state, r, s)      # (norms where the history's pointer is not: no state_hist here)
    else:
        name, extra = "gdkvm_scan_fwd", (state, r, s, state_hist)
    _call(name, dev, q, k, v, alpha, beta, *extra, _Ws(workspace), B, T, Hh, N, Dk, Dv, io, rule, flags)
    if check:
        scan_status(workspace, B, T, Hh, N, Dk, Dv, flags | (FLAG_WIDE_RANGE if rule == RULE_DELTA_PARALLEL else 0))
    return r, s


def scan_fwd_normalizer(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, alpha: torch.Tensor, beta: torch.Tensor,
                        state: Optional[torch.Tensor] = None, z: Optional[torch.Tensor] = None, rule: int = RULE_DELTA_SEQUENTIAL,
                        flags: int = 0, eps: float = 1e-6):
    """gdkvm_scan_fwd_normalizer (SURVEY.md A.1's `normalizer` flag): the scan with z [B,Hh,Dk] carried beside S and the read-out divided
    by |q . z| + eps.  Returns (R [B,T,N,Hh,Dv], S_T [B,Hh,Dk,Dv] fp32, z_T [B,Hh,Dk] fp32).  Inference only; Dk = 64."""
    B, T, N, Hh, Dk, Dv = _scan_operands(q, k, v, alpha, beta, state)
    if z is not None and (tuple(z.shape) != (B, Hh, Dk) or z.dtype != torch.float32):
        raise GdkvmError("z must be float32 [B,Hh,Dk]")
    dev = _dev(q, k, v, alpha, beta, state, z)
    io = _io_dtype(q)
    ws = _workspace("gdkvm_scan_normalizer_workspace_bytes", dev, B, T, Hh, N, Dk, Dv, io)
    r = torch.empty((B, T, N, Hh, Dv), dtype=q.dtype, device=dev)
    s = torch.empty((B, Hh, Dk, Dv), dtype=torch.float32, device=dev)
    zo = torch.empty((B, Hh, Dk), dtype=torch.float32, device=dev)
    _call("gdkvm_scan_fwd_normalizer", dev, q, k, v, alpha, beta, state, z, r, s, zo, _Ws(ws), B, T, Hh, N, Dk, Dv, io, rule, flags, float(eps))
    return r, s, zo


def lkva_read(q: torch.Tensor, state: torch.Tensor, flags: int = 0, norms: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """gdkvm_lkva_read: R [B,N,Hh,Dv] = Qn S for ONE frame per clip (the read half of a per-frame step).  q [B,N,Hh,Dk] f32|bf16,
    state [B,Hh,Dk,Dv] fp32, norms [B*N,Hh,2] fp32 from ops.proj_gates or None."""
    if q.dim() != 4 or state.dim() != 4 or state.shape[0] != q.shape[0] or state.shape[1] != q.shape[2] or state.shape[2] != q.shape[3]:
        raise GdkvmError(f"lkva_read: bad shapes q{tuple(q.shape)} state{tuple(state.shape)}")
    if state.dtype != torch.float32:
        raise GdkvmError("lkva_read: state must be float32")
    B, N, Hh, Dk = q.shape
    Dv = state.shape[-1]
    dev = _dev(q, state, norms, out)
    if norms is not None and (norms.dtype != torch.float32 or norms.numel() != B * N * Hh * 2):
        raise GdkvmError("lkva_read: norms must be float32 [B*N, Hh, 2]")
    r = _out_like(out, (B, N, Hh, Dv), q.dtype, dev, "lkva_read") if out is not None else torch.empty((B, N, Hh, Dv), dtype=q.dtype, device=dev)
    _call("gdkvm_lkva_read", dev, q, norms, state, r, B, N, Hh, Dk, Dv, _io_dtype(q), flags)
    return r


def mask_embed_add_(v: torch.Tensor, mask: torch.Tensor, w_embed: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """gdkvm_mask_embed_add, in place: v [BT, h*w, C] += w_embed[c] * adaptive_avg_pool(mask != 0) per token.  mask uint8 [BT,H,W],
    w_embed fp32 [C]."""
    if v.dim() != 3 or mask.dim() != 3 or mask.dtype != torch.uint8 or mask.shape[0] != v.shape[0] or v.shape[1] != h * w:
        raise GdkvmError(f"mask_embed_add_: bad shapes v{tuple(v.shape)} mask{tuple(mask.shape)} {mask.dtype} tokens {h}x{w}")
    if w_embed.dtype != torch.float32 or w_embed.numel() != v.shape[2]:
        raise GdkvmError("mask_embed_add_: w_embed must be float32 [C]")
    dev = _dev(v, mask, w_embed)
    _call("gdkvm_mask_embed_add", dev, mask, w_embed, v, v.shape[0], mask.shape[1], mask.shape[2], h, w, v.shape[2], _io_dtype(v))
    return v


def mask_embed_wgrad(mask: torch.Tensor, d_v: torch.Tensor, h: int, w: int, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gdkvm_mask_embed_wgrad: d_w fp32 [C] = sum over the token rows of adaptive_avg_pool(mask != 0) * d_v -- the weight gradient of
    mask_embed_add_.  mask uint8 [F,H,W], d_v [F, h*w, C] f32|bf16; workspace: uint8 of at least
    gdkvm_mask_embed_wgrad_workspace_bytes(F, h, w, C) bytes (allocated here when None)."""
    if d_v.dim() != 3 or mask.dim() != 3 or mask.dtype != torch.uint8 or mask.shape[0] != d_v.shape[0] or d_v.shape[1] != h * w:
        raise GdkvmError(f"mask_embed_wgrad: bad shapes d_v{tuple(d_v.shape)} mask{tuple(mask.shape)} {mask.dtype} tokens {h}x{w}")
    F_, C = d_v.shape[0], d_v.shape[2]
    dev = _dev(d_v, mask, workspace)
    if workspace is None:
        workspace = _workspace("gdkvm_mask_embed_wgrad_workspace_bytes", dev, F_, h, w, C, floor=16)
    dw = torch.empty(C, dtype=torch.float32, device=dev)
    _call("gdkvm_mask_embed_wgrad", dev, mask, d_v, dw, _Ws(workspace), F_, mask.shape[1], mask.shape[2], h, w, C, _io_dtype(d_v))
    return dw


class _MaskEmbedFunction(torch.autograd.Function):
    """v' = v + adaptive_avg_pool(mask != 0) (x) w_embed, differentiable in v and w_embed (training in the step mode): forward
    gdkvm_mask_embed_add on a copy of v, backward d_v = d_v' and d_w from gdkvm_mask_embed_wgrad.  The mask is a constant."""

    @staticmethod
    def forward(ctx, v, mask, weight, h, w):
        out = v.clone(memory_format=torch.contiguous_format)
        mask_embed_add_(out, mask, weight.detach().reshape(-1).float().contiguous(), h, w)
        ctx.save_for_backward(mask)
        ctx.meta = (h, w, weight.dtype, tuple(weight.shape), out.dtype)
        return out

    @staticmethod
    def backward(ctx, d_out):
        (mask,) = ctx.saved_tensors
        h, w, wdt, wshape, odt = ctx.meta
        d_out = d_out.to(odt).contiguous()
        dw = mask_embed_wgrad(mask, d_out, h, w) if ctx.needs_input_grad[2] else None
        return d_out, None, (None if dw is None else dw.reshape(wshape).to(wdt)), None, None


def mask_embed(v: torch.Tensor, mask: torch.Tensor, weight: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """v [F, h*w, C] + w_embed[c] * adaptive_avg_pool(mask != 0) per token, as a new tensor, differentiable in v and weight (C elements,
    e.g. the mask_embed 1x1 convolution's [C,1,1,1] weight): _MaskEmbedFunction.  mask uint8 [F,H,W] (255 = unlabelled = background)."""
    return _MaskEmbedFunction.apply(v, mask, weight, h, w)


def scan_status(workspace: torch.Tensor, B: int, T: int, Hh: int, N: int, Dk: int, Dv: int, flags: int = 0) -> None:
    """Raises GdkvmError (GDKVM_ERR_RANGE) if the last scan_fwd / scan_apply on ``workspace`` left the range of its fp16-pair operands
    (its results are NaNs then); returns None otherwise.  Waits for the current stream (gdkvm_scan_status)."""
    _call("gdkvm_scan_status", _dev(workspace), _Ws(workspace), B, T, Hh, N, Dk, Dv, flags)


def scan_bwd(q, k, v, alpha, beta, state_hist, workspace, d_r, d_state_out=None, rule=RULE_DELTA_SEQUENTIAL, flags=0,
             need_d_state_in=True):
    """Backward of scan_fwd (gdkvm_scan_bwd).  ``state_hist`` and ``workspace`` are the ones the forward call filled.
    Returns (d_q, d_k, d_v, d_alpha, d_beta, d_state_in | None)."""
    B, T, N, Hh, Dk = q.shape
    Dv = v.shape[-1]
    dev = _dev(q, k, v, alpha, beta, state_hist, workspace, d_r, d_state_out)
    if d_r.dtype != q.dtype or tuple(d_r.shape) != (B, T, N, Hh, Dv):
        raise GdkvmError("d_r must match the read-out's shape and dtype")
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    da = torch.empty((B, T, Hh), dtype=torch.float32, device=dev)
    db = torch.empty((B, T, N, Hh), dtype=torch.float32, device=dev)
    ds = torch.empty((B, Hh, Dk, Dv), dtype=torch.float32, device=dev) if need_d_state_in else None
    bws = _workspace("gdkvm_scan_bwd_workspace_bytes", dev, B, T, Hh, N, Dk, Dv)
    _call("gdkvm_scan_bwd", dev, q, k, v, alpha, beta, state_hist, _Ws(workspace), d_r, d_state_out, dq, dk, dv, da, db, ds, _Ws(bws),
          B, T, Hh, N, Dk, Dv, _io_dtype(q), rule, flags)
    return dq, dk, dv, da, db, ds


class _ScanFunction(torch.autograd.Function):
    """Differentiable gdkvm_scan_fwd: forward saves the state history and the WY workspace, backward is gdkvm_scan_bwd."""

    @staticmethod
    def forward(ctx, q, k, v, alpha, beta, state, rule, flags):
        B, T, N, Hh, Dk = q.shape
        Dv = v.shape[-1]
        ws = new_workspace(B, T, Hh, N, Dk, Dv, q.device)
        hist = torch.empty((B, T, Hh, Dk, Dv), dtype=torch.float32, device=q.device)
        r, s = scan_fwd(q, k, v, alpha, beta, state, rule=rule, flags=flags, workspace=ws, state_hist=hist)
        ctx.save_for_backward(q, k, v, alpha, beta, hist, ws)
        ctx.rule, ctx.flags, ctx.has_state = rule, flags, state is not None
        return r, s

    @staticmethod
    def backward(ctx, d_r, d_s):
        q, k, v, alpha, beta, hist, ws = ctx.saved_tensors
        d_r = d_r.contiguous()
        d_s = None if d_s is None else d_s.contiguous().float()
        dq, dk, dv, da, db, ds = scan_bwd(q, k, v, alpha, beta, hist, ws, d_r, d_s, ctx.rule, ctx.flags,
                                          need_d_state_in=ctx.has_state)
        return dq, dk, dv, da, db, ds, None, None


def scan_state_bwd(k, v, alpha, beta, state_hist, workspace, d_hist=None, d_state_out=None, rule=RULE_DELTA_SEQUENTIAL, flags=0,
                   need_d_state_in=True):
    """Backward of the state recurrence alone (gdkvm_scan_state_bwd): ``d_hist`` [B,T,Hh,Dk,Dv] is the gradient with respect to
    the state before every frame.  Returns (d_k, d_v, d_alpha, d_beta, d_state_in | None)."""
    B, T, N, Hh, Dk = k.shape
    Dv = v.shape[-1]
    dev = _dev(k, v, alpha, beta, state_hist, workspace, d_hist, d_state_out)
    dk, dv = torch.empty_like(k), torch.empty_like(v)
    da = torch.empty((B, T, Hh), dtype=torch.float32, device=dev)
    db = torch.empty((B, T, N, Hh), dtype=torch.float32, device=dev)
    ds = torch.empty((B, Hh, Dk, Dv), dtype=torch.float32, device=dev) if need_d_state_in else None
    bws = _workspace("gdkvm_scan_bwd_workspace_bytes", dev, B, T, Hh, N, Dk, Dv)
    _call("gdkvm_scan_state_bwd", dev, k, v, alpha, beta, state_hist, _Ws(workspace), d_hist, d_state_out, dk, dv, da, db, ds, _Ws(bws),
          B, T, Hh, N, Dk, Dv, _io_dtype(k), rule, flags)
    return dk, dv, da, db, ds


class _ReadoutFunction(torch.autograd.Function):
    """The LKVA read-out of frames of more than 64 tokens from the saved state history (gdkvm_readout_fwd), differentiable:
    the backward (gdkvm_readout_bwd) returns d_q and the gradient with respect to the states the frames read, in the history's
    own layout (what gdkvm_scan_state_bwd takes as d_hist).  gdkvm_scan_train_fwd / _bwd compose the same calls in C; this
    autograd node exposes the read-out on its own."""

    @staticmethod
    def forward(ctx, q, hist, chunks, flags):
        B, T, N, Hh, Dk = q.shape
        Dv = hist.shape[-1]
        dev = _dev(q, hist)
        if hist.dtype != torch.float32 or tuple(hist.shape) != (B, T * chunks, Hh, Dk, Dv):
            raise GdkvmError(f"state history must be float32 [B, T*chunks, Hh, Dk, Dv], got {tuple(hist.shape)}")
        r = torch.empty((B, T, N, Hh, Dv), dtype=q.dtype, device=dev)
        _call("gdkvm_readout_fwd", dev, q, hist, r, B, T, Hh, N, Dk, Dv, chunks, _io_dtype(q), flags)
        ctx.save_for_backward(q, hist)
        ctx.chunks, ctx.flags = chunks, flags
        return r

    @staticmethod
    def backward(ctx, d_r):
        q, hist = ctx.saved_tensors
        B, T, N, Hh, Dk = q.shape
        Dv = hist.shape[-1]
        d_r = d_r.contiguous()
        if d_r.dtype != q.dtype:
            d_r = d_r.to(q.dtype)
        dq = torch.empty_like(q)
        d_hist = torch.zeros_like(hist)                     # only the states before the frames receive a gradient here
        _call("gdkvm_readout_bwd", q.device, q, hist, d_r, dq, d_hist, B, T, Hh, N, Dk, Dv, ctx.chunks, _io_dtype(q), ctx.flags)
        return dq, d_hist, None, None


class _ScanTrainFunction(torch.autograd.Function):
    """Differentiable scan for frames of any token count: gdkvm_scan_train_fwd / gdkvm_scan_train_bwd, with ONE workspace carrying
    the state history, the WY factors and (N > 64) the frame re-cut into 64-token pseudo-frames from the forward to the backward
    call.  No framework op between the HIP calls."""

    @staticmethod
    def forward(ctx, q, k, v, alpha, beta, state, rule, flags):
        B, T, N, Hh, Dk = q.shape
        Dv = v.shape[-1]
        q, k, v, alpha, beta = (t.contiguous() for t in (q, k, v, alpha, beta))
        dev = _dev(q, k, v, alpha, beta, state)
        io = _io_dtype(q)
        ws = _workspace("gdkvm_scan_train_workspace_bytes", dev, B, T, Hh, N, Dk, Dv, io)
        r = torch.empty((B, T, N, Hh, Dv), dtype=q.dtype, device=dev)
        s = torch.empty((B, Hh, Dk, Dv), dtype=torch.float32, device=dev)
        _call("gdkvm_scan_train_fwd", dev, q, k, v, alpha, beta, state, r, s, _Ws(ws), B, T, Hh, N, Dk, Dv, io, rule, flags)
        ctx.save_for_backward(q, k, v, alpha, beta, ws)
        ctx.rule, ctx.flags, ctx.has_state = rule, flags, state is not None
        return r, s

    @staticmethod
    def backward(ctx, d_r, d_s):
        q, k, v, alpha, beta, ws = ctx.saved_tensors
        B, T, N, Hh, Dk = q.shape
        Dv = v.shape[-1]
        dev = q.device
        d_r = d_r.contiguous()
        if d_r.dtype != q.dtype:
            d_r = d_r.to(q.dtype)
        d_s = None if d_s is None else d_s.contiguous().float()
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        da = torch.empty((B, T, Hh), dtype=torch.float32, device=dev)
        db = torch.empty((B, T, N, Hh), dtype=torch.float32, device=dev)
        ds = torch.empty((B, Hh, Dk, Dv), dtype=torch.float32, device=dev) if ctx.has_state else None
        _call("gdkvm_scan_train_bwd", dev, q, k, v, alpha, beta, d_r, d_s, dq, dk, dv, da, db, ds, _Ws(ws), B, T, Hh, N, Dk, Dv,
              _io_dtype(q), ctx.rule, ctx.flags)
        return dq, dk, dv, da, db, ds, None, None


def scan(q, k, v, alpha, beta, state=None, rule: int = RULE_DELTA_SEQUENTIAL, flags: int = 0):
    """scan_fwd with autograd support (training).  Inference callers should use scan_fwd directly (no history)."""
    if q.shape[-1] < KERNEL_DK:                            # narrower keys (differentiable: padding and slicing are autograd ops)
        qp, kp, sp = _pad_keys(q, k, state)
        r, s = scan(qp, kp, v, alpha, beta, sp, rule, flags)
        return r, s[:, :, :q.shape[-1]]
    if q.shape[2] > 64 or q.shape[-1] > KERNEL_DK:        # (wider keys train on gdkvm_scan_train_fwd / _bwd at every N)
        return _ScanTrainFunction.apply(q, k, v, alpha, beta, state, rule, flags)
    return _ScanFunction.apply(q, k, v, alpha, beta, state, rule, flags)


def scan_prep(q, k, v, beta, workspace, rule=RULE_DELTA_SEQUENTIAL, flags=0):
    """Stage 1 of scan_fwd alone (gdkvm_scan_prep): folds every frame into its affine map S' = a P S + G in ``workspace``
    (with FLAG_TRAIN also the WY factors the backward consumes)."""
    B, T, N, Hh, Dk = k.shape
    Dv = v.shape[-1]
    dev = _dev(q, k, v, beta, workspace)
    _call("gdkvm_scan_prep", dev, q, k, v, beta, _Ws(workspace), B, T, Hh, N, Dk, Dv, _io_dtype(k), rule, flags)


def new_workspace(B, T, Hh, N, Dk, Dv, device) -> torch.Tensor:
    return _workspace("gdkvm_scan_workspace_bytes", device, B, T, Hh, N, Dk, Dv)


def scan_transition(q, alpha, workspace, Dv, flags=0):
    """State-transition matrix Phi [B,Hh,Dk,Dk] of the frames prepared in ``workspace`` (gdkvm_scan_transition):
    S_out = Phi @ S_in + S_loc for these frames."""
    B, T, N, Hh, Dk = q.shape
    dev = _dev(q, alpha, workspace)
    phi = torch.empty((B, Hh, Dk, Dk), dtype=torch.float32, device=dev)
    _call("gdkvm_scan_transition", dev, q, alpha, phi, _Ws(workspace), B, T, Hh, N, Dk, Dv, _io_dtype(q), flags)
    return phi


def scan_stitch(phi: torch.Tensor, s_loc: torch.Tensor, state: Optional[torch.Tensor] = None):
    """starts [B,S,Hh,Dk,Dv] and the end state of S consecutive segments from their transition matrices phi [B,S,Hh,Dk,Dk] and
    zero-start end states s_loc [B,S,Hh,Dk,Dv] (gdkvm_scan_stitch): starts[:,0] = state, starts[:,c+1] = phi[:,c] starts[:,c] + s_loc[:,c]."""
    B, S, Hh, Dk, Dv = s_loc.shape
    if tuple(phi.shape) != (B, S, Hh, Dk, Dk) or phi.dtype != torch.float32 or s_loc.dtype != torch.float32:
        raise GdkvmError("scan_stitch: phi [B,S,Hh,Dk,Dk] and s_loc [B,S,Hh,Dk,Dv] in float32")
    dev = _dev(phi, s_loc, state)
    phi, s_loc = phi.contiguous(), s_loc.contiguous()
    starts = torch.empty_like(s_loc)
    end = torch.empty((B, Hh, Dk, Dv), dtype=torch.float32, device=dev)
    _call("gdkvm_scan_stitch", dev, phi, s_loc, state, starts, end, B, S, Hh, Dk, Dv)
    return starts, end


def scan_fwd_segmented(q, k, v, alpha, beta, state=None, segments: int = 0, rule: int = RULE_DELTA_SEQUENTIAL, flags: int = 0,
                       workspace: Optional[torch.Tensor] = None):
    """Long-clip scan with the time axis cut into ``segments`` equal pieces that run concurrently (gdkvm_scan_fwd_segmented; SURVEY
    §8f n3 inside one GPU): per segment the transition matrix Phi_c and the zero-start end state S_loc_c, a tiny sequential
    stitch S_start_{c+1} = Phi_c S_start_c + S_loc_c, then every segment is scanned from its true start state.  2.25x the
    recurrence work on `segments`x the workgroups.  ``segments`` = 0: chosen by shape (gdkvm_scan_segments; 1 = the serial scan).
    Equal to scan_fwd up to fp32 re-association (not bit-identical)."""
    B, T, N, Hh, Dk, Dv = _scan_operands(q, k, v, alpha, beta, state)
    if segments < 0 or (segments and T % segments):
        raise GdkvmError(f"segments={segments} must divide T={T}")
    dev = _dev(q, k, v, alpha, beta, state, workspace)
    q, k, v, alpha, beta = (t.contiguous() for t in (q, k, v, alpha, beta))
    if workspace is None:                                  # (the choice by shape asks the current device for its CU count: _bytes)
        workspace = _workspace("gdkvm_scan_segmented_workspace_bytes", dev, B, T, Hh, N, Dk, Dv, segments)
    r = torch.empty((B, T, N, Hh, Dv), dtype=q.dtype, device=dev)
    s = torch.empty((B, Hh, Dk, Dv), dtype=torch.float32, device=dev)
    _call("gdkvm_scan_fwd_segmented", dev, q, k, v, alpha, beta, state, r, s, _Ws(workspace), B, T, Hh, N, Dk, Dv, segments, _io_dtype(q),
          rule, flags)
    return r, s


def scan_apply(q, alpha, workspace, Dv, state=None, flags=0, out=None, state_out=None, want_readout=True):
    """Stage 2 of scan_fwd alone (gdkvm_scan_apply): the serial read/write recurrence over a prepared workspace."""
    B, T, N, Hh, Dk = q.shape
    dev = _dev(q, alpha, workspace, state, out, state_out)
    r = None if not want_readout else (out if out is not None else torch.empty((B, T, N, Hh, Dv), dtype=q.dtype, device=dev))
    s = state_out if state_out is not None else torch.empty((B, Hh, Dk, Dv), dtype=torch.float32, device=dev)
    _call("gdkvm_scan_apply", dev, q, alpha, state, r, s, None, _Ws(workspace), B, T, Hh, N, Dk, Dv, _io_dtype(q), flags)
    return r, s


def kpff_workspace(local: torch.Tensor, glob: torch.Tensor, pixel: torch.Tensor) -> torch.Tensor:
    """A fresh workspace for kpff_fwd on these features (gdkvm_kpff_workspace_bytes): it holds the bf16 weight pack, so a caller may keep
    it and pass it back with packed=True while the weights are unchanged."""
    return _workspace("gdkvm_kpff_workspace_bytes", local.device, local.shape[-1], glob.shape[-1], pixel.shape[-1], _io_dtype(local))


def kpff_fwd(local: torch.Tensor, glob: torch.Tensor, pixel: torch.Tensor, wa: torch.Tensor, ba: torch.Tensor,
             wl: torch.Tensor, wg: torch.Tensor, h: int, w: int, out: Optional[torch.Tensor] = None,
             workspace: Optional[torch.Tensor] = None, packed: bool = False, exact: bool = False) -> torch.Tensor:
    """Key-Pixel Feature Fusion (gdkvm_kpff_fwd).  local [BT,N,Ck] glob [BT,N,Cv] pixel [BT,N,Cp], N=h*w;
    wa [2Cp,Cp+Ck+Cv] ba [2Cp] wl [Cp,Ck] wg [Cp,Cv] float32.  Returns F [BT,N,Cp] in the io dtype.
    exact (float32 features only): no workspace is handed over, which selects the exact fp32-MFMA arm instead of the arm on
    bf16 splits (include/gdkvm.h)."""
    BT, N, Ck = local.shape
    Cv, Cp = glob.shape[-1], pixel.shape[-1]
    if N != h * w or glob.shape[:2] != (BT, N) or pixel.shape[:2] != (BT, N):
        raise GdkvmError("bad KPFF feature shapes")
    if tuple(wa.shape) != (2 * Cp, Cp + Ck + Cv) or tuple(ba.shape) != (2 * Cp,) or \
            tuple(wl.shape) != (Cp, Ck) or tuple(wg.shape) != (Cp, Cv):
        raise GdkvmError("bad KPFF weight shapes")
    for t in (wa, ba, wl, wg):
        if t.dtype != torch.float32:
            raise GdkvmError("KPFF weights must be float32")
    if glob.dtype != local.dtype or pixel.dtype != local.dtype:
        raise GdkvmError("KPFF features must share one dtype")
    dev = _dev(local, glob, pixel, wa, ba, wl, wg, out, workspace)
    io = _io_dtype(local)
    f = out if out is not None else torch.empty((BT, N, Cp), dtype=local.dtype, device=dev)
    if exact:
        if local.dtype != torch.float32 or workspace is not None or packed:
            raise GdkvmError("kpff_fwd(exact=True) is the float32 arm without a workspace")
    elif workspace is None:
        workspace = kpff_workspace(local, glob, pixel)
    _call("gdkvm_kpff_fwd_packed" if packed else "gdkvm_kpff_fwd", dev,     # packed: `workspace` already holds these weights
          local, glob, pixel, wa, ba, wl, wg, f, _Ws(workspace), BT, Ck, Cv, Cp, h, w, io)
    return f


class _KpffFunction(torch.autograd.Function):
    """Differentiable KPFF: HIP forward (saving gates / mixes / pooled feature), HIP elementwise + pooling backward, and the
    six plain products of the backward on the hand-written MFMA kernels of csrc/gemm.hip."""

    @staticmethod
    def forward(ctx, local, glob, pixel, wa, ba, wl, wg, h, w):
        BT, N, Ck = local.shape
        Cv, Cp = glob.shape[-1], pixel.shape[-1]
        dev = _dev(local, glob, pixel, wa, ba, wl, wg)
        io = _io_dtype(local)
        f = torch.empty((BT, N, Cp), dtype=local.dtype, device=dev)
        gates = torch.empty((BT * N, 2 * Cp), dtype=local.dtype, device=dev)
        lp, gp = (torch.empty((BT * N, Cp), dtype=local.dtype, device=dev) for _ in range(2))
        gms = torch.empty((BT * N, Cv), dtype=local.dtype, device=dev)
        ws = kpff_workspace(local, glob, pixel)
        _call("gdkvm_kpff_fwd_train", dev, local, glob, pixel, wa, ba, wl, wg, f, gates, lp, gp, gms, _Ws(ws), BT, Ck, Cv, Cp, h, w, io)
        ctx.save_for_backward(local, pixel, wa, wl, wg, gates, lp, gp, gms)
        ctx.hw = (h, w)
        return f

    @staticmethod
    def backward(ctx, d_f):
        local, pixel, wa, wl, wg, gates, lp, gp, gms = ctx.saved_tensors
        h, w = ctx.hw
        BT, N, Ck = local.shape
        Cp, Cv = pixel.shape[-1], gms.shape[-1]
        M, dt, dev = BT * N, local.dtype, local.device
        io = _io_dtype(local)
        d_f = d_f.contiguous()
        dz = torch.empty((M, 2 * Cp), dtype=dt, device=dev)
        dlp, dgp = (torch.empty((M, Cp), dtype=dt, device=dev) for _ in range(2))
        _call("gdkvm_kpff_bwd_pre", dev, d_f, gates, lp, gp, dz, dlp, dgp, BT, N, Cp, io)
        L2, P2 = local.reshape(M, Ck), pixel.reshape(M, Cp)
        # the six products of the backward on the hand-written kernels (csrc/gemm.hip): dX-type ones as gdkvm_gemm_nt against
        # the weight with its input index leading (a one-off transpose of a small matrix), dW-type ones as gdkvm_gemm_tn
        def t_of(wt):                                       # cast and transpose in ONE copy kernel
            return torch.empty((wt.shape[1], wt.shape[0]), dtype=dt, device=dev).copy_(wt.t())
        dx = gemm_nt(dz, t_of(wa))                          # [M, Cin]
        dl_add = gemm_nt(dlp, t_of(wl))                     # [M, Ck]
        dg_add = gemm_nt(dgp, t_of(wg))                     # [M, Cv]
        # K = B*T*N tokens: split over workgroups, fp32 partials; the bias gradient (column sums of dz) rides on the first product's launch
        d_wa_p, d_ba = wgrad(dz, P2, colsum=True)
        d_wa = torch.cat([d_wa_p, wgrad(dz, L2), wgrad(dz, gms)], 1)
        d_wl = wgrad(dlp, L2)
        d_wg = wgrad(dgp, gms)
        d_p, d_l, d_g = torch.empty_like(pixel), torch.empty_like(local), torch.empty((BT, N, Cv), dtype=dt, device=dev)
        _call("gdkvm_kpff_bwd_post", dev, d_f, dx, dl_add, dg_add, d_p, d_l, d_g, BT, Ck, Cv, Cp, h, w, io)
        return d_l, d_g, d_p, d_wa, d_ba, d_wl, d_wg, None, None


def kpff(local, glob, pixel, wa, ba, wl, wg, h: int, w: int):
    """kpff_fwd with autograd support (training)."""
    return _KpffFunction.apply(local, glob, pixel, wa, ba, wl, wg, h, w)


def argmax_dice(logits: torch.Tensor, target: Optional[torch.Tensor] = None):
    """mask = argmax over classes (ties -> lowest index) and, with a target, integer Dice counts
    (gdkvm_argmax_dice).  logits [BT,ncls,H,W]; target [BT,H,W] uint8.  Returns (mask u8, counts i32|None)."""
    BT, ncls, H, W = logits.shape
    dev = _dev(logits, target)
    _u8_target(target, BT, H, W)
    mask = torch.empty((BT, H, W), dtype=torch.uint8, device=dev)
    counts = torch.empty((BT, ncls, 3), dtype=torch.int32, device=dev) if target is not None else None
    _call("gdkvm_argmax_dice", dev, logits, target, mask, counts, BT, ncls, H, W, _io_dtype(logits))
    return mask, counts


def upsample_argmax_dice(logits: torch.Tensor, H: int, W: int, target: Optional[torch.Tensor] = None,
                         mask_out: Optional[torch.Tensor] = None, counts_out: Optional[torch.Tensor] = None):
    """Fused bilinear upsample (align_corners=False) + argmax + Dice counts (gdkvm_upsample_argmax_dice).
    logits [BT,ncls,hl,wl] low-resolution; returns (mask u8 [BT,H,W], counts i32 [BT,ncls,3] | None); mask_out / counts_out: write there."""
    BT, ncls, hl, wl = logits.shape
    dev = _dev(logits, target)
    _u8_target(target, BT, H, W)
    mask = _out_like(mask_out, (BT, H, W), torch.uint8, dev, "mask_out")
    counts = _out_like(counts_out, (BT, ncls, 3), torch.int32, dev, "counts_out") if target is not None else None
    _call("gdkvm_upsample_argmax_dice", dev, logits, target, mask, counts, BT, ncls, hl, wl, H, W, _io_dtype(logits))
    return mask, counts


def _out_like(out, shape, dtype, dev, what):
    """A caller-owned output (e.g. a slice of a larger result, so that parts of a batch computed on different streams land in ONE tensor
    without a concatenation pass) or a fresh tensor."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != dev or not out.is_contiguous():
        raise GdkvmError(f"{what} must be a contiguous {dtype} tensor of shape {tuple(shape)} on the inputs' device")
    return out


def head_upsample_argmax_dice(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, H: int, W: int,
                              target: Optional[torch.Tensor] = None, mask_out: Optional[torch.Tensor] = None,
                              counts_out: Optional[torch.Tensor] = None):
    """The decoder's 1x1 head + bilinear upsample + argmax + Dice counts in one kernel (gdkvm_head_upsample_argmax_dice): x is the
    channels_last stride-4 feature [BT,C,hl,wl], weight fp32 [classes, C], bias fp32 [classes]; the class planes never reach memory.
    Bit-identical to head_logits followed by upsample_argmax_dice.  Returns (mask u8 [BT,H,W], counts i32 [BT,classes,3] | None)."""
    _channels_last("head_upsample_argmax_dice", x, shape="[BT,C,hl,wl]")
    BT, C, hl, wl = x.shape
    ncls = weight.shape[0]
    if weight.dtype != torch.float32 or bias.dtype != torch.float32 or tuple(weight.shape) != (ncls, C) or bias.numel() != ncls \
            or not weight.is_contiguous():
        raise GdkvmError("head_upsample_argmax_dice: weight fp32 [classes, C] (contiguous), bias fp32 [classes]")
    dev = _dev(weight, bias, target)                       # (x is channels_last: checked above)
    if dev != x.device:
        raise GdkvmError("all tensors must live on one device")
    _u8_target(target, BT, H, W)
    mask = _out_like(mask_out, (BT, H, W), torch.uint8, dev, "mask_out")
    counts = _out_like(counts_out, (BT, ncls, 3), torch.int32, dev, "counts_out") if target is not None else None
    _call("gdkvm_head_upsample_argmax_dice", dev, x, weight, bias, target, mask, counts, BT, C, ncls, hl, wl, H, W, _io_dtype(x))
    return mask, counts


def augment_clips(frames: torch.Tensor, target: Optional[torch.Tensor], params: torch.Tensor, frames_dtype: torch.dtype,
                  fill_label: int = 255, out: Optional[torch.Tensor] = None, target_out: Optional[torch.Tensor] = None):
    """gdkvm_augment_clips: the uint8 -> [0, 1] cast of a batch of clips with one affine warp and one intensity table per clip, and the
    labels warped alike (nearest neighbour, `fill_label` where the source lies outside the frame).  frames uint8 [B,T,C,H,W], target uint8 |
    int64 [B,T,H,W] or None, params fp32 [B,12] on the device (data.ClipAugment.params: m00 m01 m02 m10 m11 m12 gain bias gamma 0 0 0, the
    matrix mapping destination to source pixel indices), frames_dtype float32 | bfloat16.  Returns (frames_out, target_out | None); with
    the identity row the frames are torch.mul(frames, 1/255) bit for bit."""
    if frames.dtype != torch.uint8 or frames.dim() != 5:
        raise GdkvmError(f"augment_clips: frames must be uint8 [B,T,C,H,W], got {frames.dtype} {tuple(frames.shape)} (float frames are not augmented)")
    B, T, C, H, W = frames.shape
    if target is not None and (tuple(target.shape) != (B, T, H, W) or target.dtype not in (torch.uint8, torch.int64)):
        raise GdkvmError(f"augment_clips: target must be uint8 or int64 {(B, T, H, W)}, got {target.dtype} {tuple(target.shape)}")
    if params.dtype != torch.float32 or tuple(params.shape) != (B, 12):
        raise GdkvmError(f"augment_clips: params must be float32 [{B}, 12], got {params.dtype} {tuple(params.shape)}")
    if frames_dtype not in (torch.float32, torch.bfloat16):
        raise GdkvmError(f"augment_clips: frames_dtype {frames_dtype} (float32 or bfloat16)")
    if not 0 <= int(fill_label) <= 255:
        raise GdkvmError(f"augment_clips: fill_label {fill_label} outside [0, 255]")
    if target is None and target_out is not None:
        raise GdkvmError("augment_clips: target_out given without a target")
    dev = _dev(frames, target, params, out, target_out)
    f_out = _out_like(out, frames.shape, frames_dtype, dev, "augment_clips: out")
    t_out = None if target is None else _out_like(target_out, target.shape, target.dtype, dev, "augment_clips: target_out")
    if B * T > 0 and (f_out.data_ptr() == frames.data_ptr() or (target is not None and t_out.data_ptr() == target.data_ptr())):
        raise GdkvmError("augment_clips: the outputs must not alias the inputs (a gather)")
    _call("gdkvm_augment_clips", dev, frames, target, params, f_out, t_out, B, T, C, H, W, _io_dtype(f_out),
          1 if target is None else target.element_size(), int(fill_label))
    return f_out, t_out


def bias_act_(x: torch.Tensor, bias: torch.Tensor, residual: Optional[torch.Tensor] = None, relu: bool = True) -> torch.Tensor:
    """In-place fused epilogue on an NHWC (channels_last) conv output: x <- act(x + bias[c] (+ residual))  (gdkvm_bias_act)."""
    if x.dim() != 4 or not x.is_contiguous(memory_format=torch.channels_last):
        raise GdkvmError("bias_act_ needs a channels_last [N,C,H,W] tensor")
    if residual is not None and (residual.shape != x.shape or residual.dtype != x.dtype or
                                 not residual.is_contiguous(memory_format=torch.channels_last)):
        raise GdkvmError("residual must match x (shape, dtype, channels_last)")
    if bias.dtype != torch.float32 or bias.numel() != x.shape[1]:
        raise GdkvmError("bias must be float32 [C]")
    if not x.is_cuda:
        raise GdkvmError("GDKVM ops need device tensors (no CPU path)")
    n, c, hh, ww = x.shape
    _call("gdkvm_bias_act", x.device, x, bias, residual, x, n * hh * ww, c, int(relu), _io_dtype(x))
    return x


def head_logits(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """1x1 convolution + bias of a channels_last feature [N,C,H,W] to contiguous NCHW class planes [N,classes,H,W] in x's dtype
    (gdkvm_head_logits); weight fp32 [classes, C], bias fp32 [classes]."""
    _channels_last("head_logits", x)
    n, c, hh, ww = x.shape
    ncls = weight.shape[0]
    if weight.dtype != torch.float32 or bias.dtype != torch.float32 or tuple(weight.shape) != (ncls, c) or bias.numel() != ncls \
            or not weight.is_contiguous():
        raise GdkvmError("head_logits: weight fp32 [classes, C] (contiguous), bias fp32 [classes]")
    out = torch.empty((n, ncls, hh, ww), dtype=x.dtype, device=x.device)
    _call("gdkvm_head_logits", x.device, x, weight, bias, out, n, hh, ww, c, ncls, _io_dtype(x))
    return out


class _HeadFunction(torch.autograd.Function):
    """The decoder's 1x1 head in training: gdkvm_head_logits forward (NCHW class planes for the loss kernel), gdkvm_head_bwd backward
    (dx, dW, db in one pass over the feature, fixed summation order)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ncls, c = weight.shape[0], weight.shape[1]
        w2 = weight.detach().reshape(ncls, c).float().contiguous()
        b2 = bias.detach().float().contiguous()
        xc = x.contiguous(memory_format=torch.channels_last)
        ctx.save_for_backward(xc, w2)
        ctx.meta = (weight.dtype, tuple(weight.shape), bias.dtype)
        return head_logits(xc, w2, b2)

    @staticmethod
    def backward(ctx, dz):
        xc, w2 = ctx.saved_tensors
        n, c, hh, ww = xc.shape
        ncls = w2.shape[0]
        dz = dz.to(xc.dtype).contiguous()
        dx = torch.empty_like(xc)
        dw = torch.empty((ncls, c), dtype=torch.float32, device=xc.device)
        db = torch.empty(ncls, dtype=torch.float32, device=xc.device)
        ws = _workspace("gdkvm_head_bwd_workspace_bytes", xc.device, c, ncls)
        _call("gdkvm_head_bwd", xc.device, xc, dz, w2, dx, dw, db, _Ws(ws), n, hh, ww, c, ncls, _io_dtype(xc))
        wdt, wshape, bdt = ctx.meta
        return dx, dw.reshape(wshape).to(wdt), db.to(bdt)


def head_served(x: torch.Tensor, conv) -> bool:
    v = 8 if x.dtype == torch.bfloat16 else 4
    g = x.shape[1] // v if x.dim() == 4 else 0
    return (x.is_cuda and x.dim() == 4 and x.dtype in (torch.bfloat16, torch.float32) and conv.kernel_size == (1, 1) and conv.stride == (1, 1)
            and conv.padding == (0, 0) and conv.groups == 1 and conv.bias is not None and x.shape[1] % v == 0 and 0 < g <= 64 and g & (g - 1) == 0
            and conv.out_channels <= min(g, 8))


def head(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """conv2d(x, weight [classes, C, 1, 1], bias) as contiguous NCHW class planes, differentiable (training): _HeadFunction."""
    return _HeadFunction.apply(x, weight, bias)


def pack_rows_weight(weight: torch.Tensor) -> torch.Tensor:
    """W [Nout, K] (Nout a multiple of 16, K of 32) -> bf16 in the MFMA fragment order gdkvm_proj_rows streams:
    element ((ot * K/32 + ks) * 64 + lane) * 8 + j = W[16 ot + (lane & 15)][32 ks + 8 (lane >> 4) + j]."""
    nout, k = weight.shape
    if nout % 16 or k % 32:
        raise GdkvmError("pack_rows_weight: [Nout, K] with Nout % 16 == 0 and K % 32 == 0")
    w = weight.detach().reshape(nout // 16, 16, k // 32, 4, 8)            # [ot, i, ks, g, j]
    return w.permute(0, 2, 3, 1, 4).contiguous().to(torch.bfloat16).reshape(-1)       # [ot, ks, g, i, j]: lane = 16 g + i


def proj_rows(x2d: torch.Tensor, wpack: torch.Tensor, bias: torch.Tensor, widths) -> Tuple[torch.Tensor, ...]:
    """The key / query / value projections of token rows x2d [rows, K] (bf16) in one pass (gdkvm_proj_rows): returns one
    contiguous [rows, w] tensor per entry of `widths` (up to three)."""
    if x2d.dim() != 2 or not x2d.is_cuda or x2d.dtype != torch.bfloat16 or not x2d.is_contiguous():
        raise GdkvmError("proj_rows needs a contiguous bf16 [rows, K] device tensor (no CPU path)")
    rows, k = x2d.shape
    widths = list(widths) + [0] * (3 - len(widths))
    if len(widths) != 3 or bias.dtype != torch.float32 or bias.numel() != sum(widths) or wpack.dtype != torch.bfloat16 \
            or wpack.numel() != sum(widths) * k:
        raise GdkvmError("proj_rows: up to three widths, fp32 bias [sum(widths)], packed bf16 weight [sum(widths) * K]")
    outs = [torch.empty((rows, w), dtype=x2d.dtype, device=x2d.device) if w else None for w in widths]
    _call("gdkvm_proj_rows", x2d.device, x2d, wpack, bias, *outs, rows, k, *widths, BF16)
    return tuple(o for o in outs if o is not None)


def gate_logits(p_tok: torch.Tensor, w_gate: torch.Tensor, b_gate: torch.Tensor, w_decay: torch.Tensor, b_decay: torch.Tensor):
    """(beta_logit [F,N,Hh], alpha_logit [F,Hh]) in fp32 from the pixel feature p_tok [F,N,Cp] in one pass (gdkvm_gate_logits):
    the gate projection per token and the decay projection of the token mean."""
    if p_tok.dim() != 3 or not p_tok.is_cuda or not p_tok.is_contiguous():
        raise GdkvmError("gate_logits needs a contiguous [frames, N, Cp] device tensor (no CPU path)")
    fr, n, cp = p_tok.shape
    hh = w_gate.shape[0]
    ws = [t.detach().float().contiguous() for t in (w_gate.reshape(hh, -1), b_gate, w_decay.reshape(hh, -1), b_decay)]
    if ws[0].shape != (hh, cp) or ws[2].shape != (hh, cp) or ws[1].numel() != hh or ws[3].numel() != hh:
        raise GdkvmError("gate_logits: weights must be [Hh, Cp], biases [Hh]")
    beta = torch.empty((fr, n, hh), dtype=torch.float32, device=p_tok.device)
    alpha = torch.empty((fr, hh), dtype=torch.float32, device=p_tok.device)
    _call("gdkvm_gate_logits", p_tok.device, p_tok, *ws, beta, alpha, fr, n, cp, hh, _io_dtype(p_tok))
    return beta, alpha


def proj_gates(p_tok: torch.Tensor, wpack: torch.Tensor, bias: torch.Tensor, w_gate: torch.Tensor, b_gate: torch.Tensor,
               w_decay: torch.Tensor, b_decay: torch.Tensor, heads: int, key_dim: int, value_dim: int):
    """Everything the memory path derives from the stride-16 pixel feature p_tok [frames, N, Cp] (bf16) in ONE launch
    (gdkvm_proj_gates): returns (k [rows, Hh*Dk], q [rows, Hh*Dk], v [rows, Hh*Dv]) in bf16, (beta_logit [frames, N, Hh],
    alpha_logit [frames, Hh]) in fp32, and norms [rows, Hh, 2] fp32 -- the inverse L2 norms of the stored key / query rows, which
    scan_fwd(..., norms=norms) takes instead of computing them.  wpack / bias: pack_rows_weight of the stacked key, query, value
    weights and their fp32 biases; gate weights fp32 [Hh, Cp]."""
    if p_tok.dim() != 3 or not p_tok.is_cuda or p_tok.dtype != torch.bfloat16 or not p_tok.is_contiguous():
        raise GdkvmError("proj_gates needs a contiguous bf16 [frames, N, Cp] device tensor (no CPU path)")
    fr, n, cp = p_tok.shape
    wk, wv = heads * key_dim, heads * value_dim
    gw = [t.detach().float().contiguous() for t in (w_gate.reshape(heads, -1), b_gate, w_decay.reshape(heads, -1), b_decay)]
    if gw[0].shape != (heads, cp) or gw[2].shape != (heads, cp) or gw[1].numel() != heads or gw[3].numel() != heads:
        raise GdkvmError("proj_gates: gate weights must be [Hh, Cp], biases [Hh]")
    if bias.dtype != torch.float32 or bias.numel() != 2 * wk + wv or wpack.dtype != torch.bfloat16 or wpack.numel() != (2 * wk + wv) * cp:
        raise GdkvmError("proj_gates: packed bf16 weight [(2 Hh Dk + Hh Dv) * Cp] and fp32 bias [2 Hh Dk + Hh Dv]")
    dev, rows = p_tok.device, fr * n
    k, q = (torch.empty((rows, wk), dtype=p_tok.dtype, device=dev) for _ in range(2))
    v = torch.empty((rows, wv), dtype=p_tok.dtype, device=dev)
    beta = torch.empty((fr, n, heads), dtype=torch.float32, device=dev)
    alpha = torch.empty((fr, heads), dtype=torch.float32, device=dev)
    norms = torch.empty((rows, heads, 2), dtype=torch.float32, device=dev)
    _call("gdkvm_proj_gates", dev, p_tok, wpack, bias, k, q, v, *gw, beta, alpha, norms, fr, n, cp, heads, key_dim, value_dim, BF16)
    return (k, q, v), (beta, alpha), norms


CONV_PACKED_WEIGHTS = 32


def conv3x3_pack_weights(weight: torch.Tensor) -> torch.Tensor:
    """The fragment-ordered copy of channels_last bf16 [K,C,3,3] weights that conv_bias_act(..., packed=...) reads
    (gdkvm_conv3x3_pack_weights): K a multiple of 16, C of 64.  Same bytes, another order; keep it next to the weights."""
    if weight.dim() != 4 or weight.dtype != torch.bfloat16 or tuple(weight.shape[2:]) != (3, 3) or not weight.is_cuda or \
            not weight.is_contiguous(memory_format=torch.channels_last):
        raise GdkvmError("conv3x3_pack_weights: weight must be a channels_last bf16 [K,C,3,3] device tensor")
    k, c = weight.shape[:2]
    packed = torch.empty(k * 9 * c, dtype=torch.bfloat16, device=weight.device)
    _call("gdkvm_conv3x3_pack_weights", weight.device, weight, packed, k, c, BF16)
    return packed


CONV_KERNEL_IGEMM = 9         # gdkvm_conv_bias_act's general implicit-GEMM kernel (any R x S / stride / pad; packed weights only)


def conv_igemm_pack_weights(weight: torch.Tensor) -> torch.Tensor:
    """The fragment-ordered copy of channels_last bf16 [K,C,R,S] weights that conv_bias_act(..., tile=CONV_KERNEL_IGEMM, packed=...)
    reads (gdkvm_conv_igemm_pack_weights): K a multiple of 16 (128 for the kernel), C of 32."""
    _channels_last("conv_igemm_pack_weights: the weight", weight, dtype=torch.bfloat16, shape="[K,C,R,S]")
    k, c, r, s = weight.shape
    packed = torch.empty(weight.numel(), dtype=torch.bfloat16, device=weight.device)
    _call("gdkvm_conv_igemm_pack_weights", weight.device, weight, packed, k, c, r, s, BF16)
    return packed


def conv_down_bias_act(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, packed: torch.Tensor, down_weight: torch.Tensor,
                       down_packed: torch.Tensor, down_bias: Optional[torch.Tensor] = None, stride: int = 2, relu: bool = True):
    """A residual block's first convolution and its 1x1 downsample branch in one launch (gdkvm_conv_down_bias_act):
    (act(conv(x, weight, stride, pad = R // 2) + bias), conv(x, down_weight, stride) (+ down_bias)); channels_last bf16, the packs as
    conv_igemm_pack_weights made them."""
    _channels_last("conv_down_bias_act", x, dtype=torch.bfloat16)
    n, c, hh, ww = x.shape
    k, _, r, s = weight.shape
    if tuple(down_weight.shape) != (k, c, 1, 1) or weight.shape[1] != c or packed.numel() != weight.numel() or down_packed.numel() != k * c \
            or packed.dtype != torch.bfloat16 or down_packed.dtype != torch.bfloat16:
        raise GdkvmError("conv_down_bias_act: weight [K,C,R,R], down_weight [K,C,1,1] and their conv_igemm_pack_weights copies")
    if bias.dtype != torch.float32 or bias.numel() != k or (down_bias is not None and (down_bias.dtype != torch.float32 or down_bias.numel() != k)):
        raise GdkvmError("biases must be float32 [K]")
    pad = r // 2
    ho, wo = (hh + 2 * pad - r) // stride + 1, (ww + 2 * pad - s) // stride + 1
    y = torch.empty((n, k, ho, wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    yd = torch.empty_like(y)
    _call("gdkvm_conv_down_bias_act", x.device, x, packed, bias, y, int(relu), down_packed, down_bias, yd, n, c, hh, ww, k, r, s, stride, pad, BF16)
    return y, yd


def _conv3x3_packed(x: torch.Tensor, packed: torch.Tensor, k_out: int, bias: torch.Tensor, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """conv3x3 / stride 1 / pad 1 of channels_last bf16 x with weights given ONLY as a pack (no epilogue beyond the bias and an optional
    residual [N, k_out, H, W] of x's type added in the kernel's epilogue)."""
    n, c, hh, ww = x.shape
    y = torch.empty((n, k_out, hh, ww), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    _call("gdkvm_conv_bias_act", x.device, x, packed, bias, residual, y, n, c, hh, ww, k_out, 3, 3, 1, 1, 0, CONV_PACKED_WEIGHTS, BF16)
    return y


_ZERO_BIAS = {}


def _zero_bias(k: int, device) -> torch.Tensor:
    key = (k, str(device))
    if key not in _ZERO_BIAS:
        _ZERO_BIAS[key] = torch.zeros(k, dtype=torch.float32, device=device)
    return _ZERO_BIAS[key]


# The training step's weight packs live ON the parameter (``w._gdkvm_train_packs``), not in a table keyed by id(): they go when the parameter
# goes, and a new parameter that reuses the id / address of a dead one cannot inherit them.  They are valid only inside the PACK SCOPE they were
# made for (``train_packs``: one forward of one model) -- NOT "until the version counter changes": torch.optim.AdamW(fused=True) writes the
# parameters without bumping ``_version`` (round 5: keyed on the counter, the fourteen stride-1 3x3 layers kept convolving with their initial
# weights under the fused optimiser, and the loss fell ~10x slower than under the default one).
_PACK_SCOPE = [None]
_PACK_TOKENS = [0]


def conv3x3_train_packs(weights) -> int:
    """Both packs (forward, data gradient) of every listed fp32 [K,C,3,3] weight in ONE launch (gdkvm_conv3x3_pack_weights_train), into
    buffers kept on the parameter; EVERY call re-packs every weight (a fused optimiser step leaves no trace a cache could key on) and opens a
    new pack scope: ops.conv3x3 uses a weight's packs only while the scope of the call that made them is open (``end_train_packs`` closes it;
    ``train_packs`` is the context-manager form).  Returns the number of layers packed."""
    todo = []
    _PACK_TOKENS[0] += 1
    token = _PACK_TOKENS[0]
    for w in weights:
        k, c = w.shape[:2]
        if not (w.is_cuda and w.dtype == torch.float32 and w.dim() == 4 and tuple(w.shape[2:]) == (3, 3) and k % 64 == 0 and c % 64 == 0):
            continue
        ent = w.__dict__.get("_gdkvm_train_packs")
        if ent is None or ent[1].numel() != k * 9 * c or ent[1].device != w.device:
            ent = (None, torch.empty(k * 9 * c, dtype=torch.bfloat16, device=w.device), torch.empty(k * 9 * c, dtype=torch.bfloat16, device=w.device))
        w.__dict__["_gdkvm_train_packs"] = ((token, w._version, w.data_ptr(), tuple(w.stride())), ent[1], ent[2])
        todo.append(w)
    for i0 in range(0, len(todo), 24):
        part = todo[i0:i0 + 24]
        n = len(part)
        P = ctypes.c_void_p * n
        wp = P(*[w.data_ptr() for w in part])
        fp = P(*[w.__dict__["_gdkvm_train_packs"][1].data_ptr() for w in part])
        dp = P(*[w.__dict__["_gdkvm_train_packs"][2].data_ptr() for w in part])
        ks = (ctypes.c_int * n)(*[w.shape[0] for w in part])
        cs = (ctypes.c_int * n)(*[w.shape[1] for w in part])
        st = (ctypes.c_longlong * (4 * n))(*[x for w in part for x in w.stride()])
        _call("gdkvm_conv3x3_pack_weights_train", part[0].device, n, *(ctypes.cast(a, ctypes.c_void_p) for a in (wp, fp, dp, ks, cs, st)))
    _PACK_SCOPE[0] = token
    return len(todo)


def end_train_packs() -> None:
    """Close the pack scope conv3x3_train_packs opened (the end of the forward it was opened for)."""
    _PACK_SCOPE[0] = None


class train_packs:
    """``with ops.train_packs(weights): ...`` -- conv3x3_train_packs for the block, the scope closed at its end."""

    def __init__(self, weights):
        self.weights = list(weights)

    def __enter__(self):
        self.packed = conv3x3_train_packs(self.weights)
        return self

    def __exit__(self, *exc):
        end_train_packs()
        return False


def drop_train_packs(weights) -> None:
    for w in weights:
        w.__dict__.pop("_gdkvm_train_packs", None)


def _train_packs_of(weight):
    ent = weight.__dict__.get("_gdkvm_train_packs")
    if ent is not None and _PACK_SCOPE[0] is not None and ent[0] == (_PACK_SCOPE[0], weight._version, weight.data_ptr(), tuple(weight.stride())):
        return ent[1], ent[2]
    return None


class _Conv3x3Function(torch.autograd.Function):
    """Training-mode 3x3 / stride 1 / pad 1 convolution (no bias) on the hand-written kernels: forward, the data gradient (the
    same kernel on the flipped, transposed weights: gdkvm_conv3x3_pack_weights_dgrad) and the weight gradient
    (gdkvm_conv3x3_wgrad).  bf16 activations (autocast), fp32 master weights."""

    @staticmethod
    def forward(ctx, x, weight, fork=False):
        xb = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        k, c = weight.shape[:2]
        ctx.fork = bool(fork)
        if fork:
            # conv3x3_fork: a second output that IS the input (for the residual branch of the block).  Its gradient then arrives HERE, together
            # with the convolution's, and is added in the data-gradient kernel's epilogue instead of by a separate pass over both tensors
            y, dummy = _Conv3x3Function._fwd(ctx, x, xb, weight, k, c)
            return y, xb.view(xb.shape)
        return _Conv3x3Function._fwd(ctx, x, xb, weight, k, c)[0]

    @staticmethod
    def _fwd(ctx, x, xb, weight, k, c):
        packs = _train_packs_of(weight)                    # (conv3x3_train_packs ran for this version of the weight: nothing to cast or pack here)
        ctx.kc, ctx.wdtype, ctx.xdtype = (k, c), weight.dtype, x.dtype
        ctx.w_cl = weight.is_contiguous(memory_format=torch.channels_last) and not weight.is_contiguous()
        if packs is not None:
            # the data-gradient pack belongs to THIS version of the weight: a copy would cost what the pre-pack saves, so the backward
            # checks that the weight has not been written since (an optimiser step between forward and backward is not a thing)
            ctx.dgrad_pack, ctx.pack_key = packs[1], (weight._version, weight.data_ptr())
            ctx.save_for_backward(xb, weight)              # (the weight rides along only to be checked in the backward: autograd tracks it)
            return _conv3x3_packed(xb, packs[0], k, _zero_bias(k, xb.device)), None
        wb = weight.detach().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        packed = torch.empty(k * 9 * c, dtype=torch.bfloat16, device=xb.device)
        _call("gdkvm_conv3x3_pack_weights", xb.device, wb, packed, k, c, BF16)
        ctx.dgrad_pack = None
        ctx.save_for_backward(xb, wb)
        return _conv3x3_packed(xb, packed, k, _zero_bias(k, xb.device)), None

    @staticmethod
    def backward(ctx, dy, d_alias=None):
        k, c = ctx.kc
        dyb = dy.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        res = None if d_alias is None else d_alias.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        dx = dw = None
        if ctx.dgrad_pack is not None:
            (xb, w), wb = ctx.saved_tensors, None           # (an in-place write of the weight since the forward makes saved_tensors itself raise)
            if (w._version, w.data_ptr()) != ctx.pack_key:
                raise RuntimeError("conv3x3: the weight was modified between forward and backward (its pre-packed data-gradient copy is stale)")
        else:
            xb, wb = ctx.saved_tensors
        if ctx.needs_input_grad[0]:
            packed = ctx.dgrad_pack
            if packed is None:
                packed = torch.empty(k * 9 * c, dtype=torch.bfloat16, device=dyb.device)
                _call("gdkvm_conv3x3_pack_weights_dgrad", dyb.device, wb, packed, k, c, BF16)
            dx = _conv3x3_packed(dyb, packed, c, _zero_bias(c, dyb.device), res).to(ctx.xdtype)
        elif res is not None:
            dx = res.to(ctx.xdtype)
        if ctx.needs_input_grad[1]:
            dw = conv3x3_wgrad(xb, dyb, channels_last=ctx.w_cl).to(ctx.wdtype)  # (fp32 sums over all pixels, deterministic; in the weight's own memory order)
        return dx, dw, None


def conv3x3_wgrad(x: torch.Tensor, dy: torch.Tensor, channels_last: bool = False) -> torch.Tensor:
    """dW [K,C,3,3] fp32 of a 3x3 / stride 1 / pad 1 convolution from channels_last bf16 x [N,C,H,W] and dy [N,K,H,W]
    (gdkvm_conv3x3_wgrad): C, K multiples of 64, rows of at most 64 pixels; deterministic.  channels_last: the result in the memory
    order of a channels_last parameter (gdkvm_conv3x3_wgrad_krsc) -- the same numbers, no re-layout copy when it becomes that
    parameter's .grad."""
    _channels_last("conv3x3_wgrad", x, dy, dtype=torch.bfloat16)
    n, c, hh, ww = x.shape
    k = dy.shape[1]
    if tuple(dy.shape) != (n, k, hh, ww):
        raise GdkvmError("conv3x3_wgrad: x and dy must agree in batch and size")
    dw = torch.empty((k, c, 3, 3), dtype=torch.float32, device=x.device, memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    ws = _grown_workspace("gdkvm_conv3x3_wgrad_workspace_bytes", x.device, n, c, hh, ww, k)      # (grown to the largest layer: up to 75 MB of partial blocks)
    _call("gdkvm_conv3x3_wgrad_krsc" if channels_last else "gdkvm_conv3x3_wgrad", x.device, x, dy, dw, _Ws(ws), n, c, hh, ww, k, BF16)
    return dw


def conv3x3_train_served(x: torch.Tensor, weight: torch.Tensor, stride, padding, dilation, groups) -> bool:
    """Does conv3x3 (forward + data gradient on the hand-written kernels) serve this layer and input?"""
    k, c = weight.shape[:2]
    return (x.is_cuda and x.dim() == 4 and tuple(weight.shape[2:]) == (3, 3) and tuple(stride) == (1, 1) and tuple(padding) == (1, 1)
            and tuple(dilation) == (1, 1) and groups == 1 and c % 64 == 0 and k % 64 == 0 and x.shape[-1] <= 64
            and (x.dtype == torch.bfloat16 or (torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16)))


def conv3x3(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """conv2d(x, weight, padding=1) for a 3x3 / stride-1 layer with channel counts in multiples of 64, differentiable, bf16."""
    return _Conv3x3Function.apply(x, weight)


def conv3x3_fork(x: torch.Tensor, weight: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(conv3x3(x, weight), x') where x' is x itself (bf16, channels_last) as a second output of the same autograd node: a residual block
    feeds x' to its skip connection, and the skip's gradient is then added to the convolution's data gradient inside that kernel's
    epilogue (its residual input) instead of by the framework's add over two full tensors."""
    return _Conv3x3Function.apply(x, weight, True)


def conv_wgrad_strided(x: torch.Tensor, dy: torch.Tensor, weight_like: torch.Tensor, stride: int, pad: int) -> torch.Tensor:
    """dW (fp32, in `weight_like`'s shape [K,C,R,S] AND memory format) of conv2d(x, w, stride, pad) from channels_last bf16 x [N,C,H,W] and
    dy [N,K,Ho,Wo] (gdkvm_conv_wgrad_strided): any window / stride / pad, C a multiple of 64, K of 8; fixed-order sums -- the same bits on
    every run."""
    _channels_last("conv_wgrad_strided", x, dy, dtype=torch.bfloat16)
    n, c, hh, ww = x.shape
    k, c2, r, s_ = weight_like.shape
    ho, wo = (hh + 2 * pad - r) // stride + 1, (ww + 2 * pad - s_) // stride + 1
    if c2 != c or tuple(dy.shape) != (n, k, ho, wo):
        raise GdkvmError(f"conv_wgrad_strided: x {tuple(x.shape)}, dy {tuple(dy.shape)} and weight {tuple(weight_like.shape)} do not fit stride {stride} pad {pad}")
    dw = torch.empty_strided(tuple(weight_like.shape), tuple(weight_like.stride()), dtype=torch.float32, device=x.device)
    ws = _grown_workspace("gdkvm_conv_wgrad_strided_workspace_bytes", x.device, n, c, hh, ww, k, r, s_, stride, pad)     # (the largest layer: ~30 MB)
    _call("gdkvm_conv_wgrad_strided", x.device, x, dy, dw, *dw.stride(), _Ws(ws), n, c, hh, ww, k, r, s_, stride, pad, BF16)
    return dw


def conv_s2_packs(weight: torch.Tensor, down_weight: Optional[torch.Tensor]):
    """(forward pack, forward pack of the 1x1 branch | None, data-gradient pack) of a [K,C,3,3] fp32 weight and its block's [K,C,1,1] branch,
    ONE launch from the master weights in whatever memory format they have (gdkvm_conv_s2_pack_train)."""
    k, c = weight.shape[:2]
    if weight.dtype != torch.float32 or tuple(weight.shape[2:]) != (3, 3) or not weight.is_cuda:
        raise GdkvmError("conv_s2_packs: fp32 [K,C,3,3] device weight")
    if down_weight is not None and (tuple(down_weight.shape) != (k, c, 1, 1) or down_weight.dtype != torch.float32 or down_weight.device != weight.device):
        raise GdkvmError("conv_s2_packs: the branch weight must be fp32 [K,C,1,1] on the same device")
    dev = weight.device
    fwd = torch.empty(k * 9 * c, dtype=torch.bfloat16, device=dev)
    fwd_d = None if down_weight is None else torch.empty(k * c, dtype=torch.bfloat16, device=dev)
    dg = torch.empty(_bytes("gdkvm_conv_s2_dgrad_pack_bytes", dev, c, k, int(down_weight is not None)) // 2, dtype=torch.bfloat16, device=dev)
    st = (ctypes.c_longlong * 4)(*weight.stride())
    sd = None if down_weight is None else (ctypes.c_longlong * 2)(*down_weight.stride()[:2])
    _call("gdkvm_conv_s2_pack_train", dev, weight, ctypes.cast(st, ctypes.c_void_p), down_weight,
          None if sd is None else ctypes.cast(sd, ctypes.c_void_p), fwd, fwd_d, dg, k, c)
    return fwd, fwd_d, dg


class _ConvS2BlockFunction(torch.autograd.Function):
    """A residual block's 3x3 / stride-2 / pad-1 convolution and its 1x1 / stride-2 downsample branch as ONE autograd node on the hand-written
    kernels (csrc/conv_s2_train.hip): (y, y_down) forward from one launch, one data-gradient launch for both branches (the framework would add
    two full-size gradients of the block's input), two deterministic weight gradients.  bf16 activations, fp32 master weights."""

    @staticmethod
    def forward(ctx, x, weight, down_weight):
        xb = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        n, c, hh, ww = xb.shape
        k = weight.shape[0]
        fwd, fwd_d, dg = conv_s2_packs(weight.detach(), down_weight.detach())
        ho, wo = (hh - 1) // 2 + 1, (ww - 1) // 2 + 1
        y = torch.empty((n, k, ho, wo), dtype=torch.bfloat16, device=xb.device, memory_format=torch.channels_last)
        yd = torch.empty_like(y)
        _call("gdkvm_conv_down_bias_act", xb.device, xb, fwd, _zero_bias(k, xb.device), y, 0, fwd_d, None, yd, n, c, hh, ww, k, 3, 3, 2, 1, BF16)
        ctx.save_for_backward(xb, dg, weight, down_weight)
        ctx.xdtype = x.dtype
        return y, yd

    @staticmethod
    def backward(ctx, dy, dyd):
        xb, dg, weight, down_weight = ctx.saved_tensors
        n, c, hh, ww = xb.shape
        k = weight.shape[0]
        cl = torch.channels_last
        dyb = dy.to(torch.bfloat16).contiguous(memory_format=cl)
        dydb = dyd.to(torch.bfloat16).contiguous(memory_format=cl)
        dx = dw = dwd = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(xb)
            _call("gdkvm_conv_s2_dgrad", xb.device, dyb, dydb, dg, dx, n, c, hh, ww, k, 1, BF16)
            dx = dx.to(ctx.xdtype)
        if ctx.needs_input_grad[1]:
            dw = conv_wgrad_strided(xb, dyb, weight, 2, 1).to(weight.dtype)
        if ctx.needs_input_grad[2]:
            dwd = conv_wgrad_strided(xb, dydb, down_weight, 2, 0).to(down_weight.dtype)
        return dx, dw, dwd


def conv_s2_block_served(x: torch.Tensor, conv, down) -> bool:
    """Does conv_s2_block serve this residual block's (3x3 / stride-2 convolution, 1x1 / stride-2 branch) pair on this input?"""
    w = conv.weight
    k, c = w.shape[:2]
    return (x.is_cuda and x.dim() == 4 and conv.bias is None and down.bias is None and tuple(w.shape[2:]) == (3, 3)
            and tuple(conv.stride) == (2, 2) and tuple(conv.padding) == (1, 1) and tuple(conv.dilation) == (1, 1) and conv.groups == 1
            and conv.padding_mode == "zeros" and tuple(down.weight.shape) == (k, c, 1, 1) and tuple(down.stride) == (2, 2)
            and tuple(down.padding) == (0, 0) and down.groups == 1 and c % 64 == 0 and k % 128 == 0
            and w.dtype == torch.float32 and down.weight.dtype == torch.float32
            and (x.dtype == torch.bfloat16 or (torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16)))


def conv_s2_block(x: torch.Tensor, weight: torch.Tensor, down_weight: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(conv2d(x, weight, stride 2, padding 1), conv2d(x, down_weight, stride 2)) in bf16, differentiable, deterministic."""
    return _ConvS2BlockFunction.apply(x, weight, down_weight)


def conv_bias_act(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, residual: Optional[torch.Tensor] = None,
                  stride: int = 1, padding: int = 1, relu: bool = True, tile: int = 0,
                  packed: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(conv2d(x, weight) + bias[k] (+ residual)) as ONE kernel on channels_last bf16 tensors (gdkvm_conv_bias_act): the
    epilogue runs on the fp32 accumulator inside the implicit-GEMM kernel, no second pass over the output.  packed: the
    conv3x3_pack_weights copy of `weight` (kernel 5 reads it instead: faster, same result)."""
    _channels_last("conv_bias_act", x, dtype=torch.bfloat16)
    if weight.dim() != 4 or weight.dtype != torch.bfloat16 or weight.shape[1] != x.shape[1] or \
            not weight.is_contiguous(memory_format=torch.channels_last):
        raise GdkvmError("conv_bias_act: weight must be channels_last bf16 [K,C,R,S]")
    n, c, hh, ww = x.shape
    k, _, r, s = weight.shape
    if bias.dtype != torch.float32 or bias.numel() != k:
        raise GdkvmError("bias must be float32 [K]")
    ho, wo = (hh + 2 * padding - r) // stride + 1, (ww + 2 * padding - s) // stride + 1
    y = torch.empty((n, k, ho, wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    if residual is not None and (residual.shape != y.shape or residual.dtype != y.dtype or
                                 not residual.is_contiguous(memory_format=torch.channels_last)):
        raise GdkvmError("residual must match the output (shape, dtype, channels_last)")
    if packed is not None:
        if packed.dtype != torch.bfloat16 or packed.numel() != weight.numel() or packed.device != x.device:
            raise GdkvmError("conv_bias_act: packed must be conv3x3_pack_weights(weight)")
        tile |= CONV_PACKED_WEIGHTS
    _call("gdkvm_conv_bias_act", x.device, x, packed if packed is not None else weight, bias, residual, y,
          n, c, hh, ww, k, r, s, stride, padding, int(relu), tile, BF16)
    return y


def bias_relu_maxpool(x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """relu(max_pool2d(x, 3, 2, 1) + bias[c]) on a channels_last conv output in one pass (gdkvm_bias_relu_maxpool);
    equals max_pool2d(relu(x + bias), 3, 2, 1).  x may be a top-left spatial crop (a view) of a larger channels_last tensor."""
    if x.dim() != 4 or not x.is_cuda:
        raise GdkvmError("bias_relu_maxpool needs a channels_last [N,C,H,W] device tensor (or a spatial crop of one)")
    n, c, hh, ww = x.shape
    if x.is_contiguous(memory_format=torch.channels_last):
        x_rows, x_cols = hh, ww
    else:                                                   # a top-left spatial crop: the strides carry the stored size
        sn, sc, sh, sw = x.stride()
        if sc != 1 or sw != c or sh % c or (n > 1 and sn % sh):
            raise GdkvmError("bias_relu_maxpool needs a channels_last [N,C,H,W] device tensor (or a spatial crop of one)")
        x_cols = sh // c
        x_rows = sn // sh if n > 1 else hh
    if bias.dtype != torch.float32 or bias.numel() != c:
        raise GdkvmError("bias must be float32 [C]")
    out = torch.empty((n, c, (hh - 1) // 2 + 1, (ww - 1) // 2 + 1), device=x.device, dtype=x.dtype,
                      memory_format=torch.channels_last)
    _call("gdkvm_bias_relu_maxpool", x.device, x, bias, out, n, hh, ww, c, x_rows, x_cols, _io_dtype(x))
    return out


def stem_s2d(x: torch.Tensor, cpad: int) -> torch.Tensor:
    """Space-to-depth of NCHW frames for the stem: [N,C,H,W] contiguous -> channels_last [N,cpad,H/2,W/2] with channel
    (c*2+p)*2+q = x[c, 2i+p, 2j+q] and zeros above 4C (gdkvm_stem_s2d)."""
    if x.dim() != 4 or not x.is_cuda or not x.is_contiguous():
        raise GdkvmError("stem_s2d needs a contiguous NCHW device tensor")
    n, c, hh, ww = x.shape
    out = torch.empty((n, cpad, hh // 2, ww // 2), device=x.device, dtype=x.dtype, memory_format=torch.channels_last)
    _call("gdkvm_stem_s2d", x.device, x, out, n, c, hh, ww, cpad, _io_dtype(x))
    return out


def upsample_bilinear(lo: torch.Tensor, size) -> torch.Tensor:
    """F.interpolate(lo, size, mode="bilinear", align_corners=False) on a channels_last bf16 [N,C,h,w] device tensor
    (gdkvm_upsample_cat without a skip tensor): what conv_cat_bias_act reads next to the skip feature."""
    _channels_last("upsample_bilinear", lo, dtype=torch.bfloat16, shape="[N,C,h,w]")
    n, c1, hl, wl = lo.shape
    H, W = int(size[0]), int(size[1])
    out = torch.empty((n, c1, H, W), dtype=lo.dtype, device=lo.device, memory_format=torch.channels_last)
    _call("gdkvm_upsample_cat", lo.device, lo, None, out, n, hl, wl, H, W, c1, 0, BF16)
    return out


def _conv_cat_operands(what: str, x1, x2, size, weight, bias, residual, packed) -> torch.Tensor:
    """The checks conv_cat_bias_act and conv_upcat_bias_act share (x1 is the tensor whose channels come first; size = x2's map); returns
    the empty output."""
    _channels_last(what, x1, x2, dtype=torch.bfloat16)
    n, c1 = x1.shape[:2]
    c2, hh, ww = x2.shape[1:]
    if x2.shape[0] != n or tuple(size) != (hh, ww):
        raise GdkvmError(f"{what}: the two inputs must agree in batch and size")
    if weight.dim() != 4 or weight.dtype != torch.bfloat16 or tuple(weight.shape[1:]) != (c1 + c2, 3, 3) or \
            not weight.is_contiguous(memory_format=torch.channels_last):
        raise GdkvmError(f"{what}: weight must be channels_last bf16 [K,C1+C2,3,3]")
    k = weight.shape[0]
    if bias.dtype != torch.float32 or bias.numel() != k:
        raise GdkvmError("bias must be float32 [K]")
    y = torch.empty((n, k, hh, ww), dtype=x1.dtype, device=x1.device, memory_format=torch.channels_last)
    if residual is not None and (residual.shape != y.shape or residual.dtype != y.dtype or
                                 not residual.is_contiguous(memory_format=torch.channels_last)):
        raise GdkvmError("residual must match the output (shape, dtype, channels_last)")
    if packed is not None and (packed.dtype != torch.bfloat16 or packed.numel() != weight.numel() or packed.device != x1.device):
        raise GdkvmError(f"{what}: packed must be conv3x3_pack_weights(weight)")
    return y


def conv_cat_bias_act(x1: torch.Tensor, x2: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
                      residual: Optional[torch.Tensor] = None, relu: bool = True, tile: int = 0,
                      packed: Optional[torch.Tensor] = None) -> torch.Tensor:
    """conv_bias_act(torch.cat([x1, x2], 1), weight, ...) for a 3x3 / stride 1 / pad 1 layer WITHOUT the concatenated tensor
    (gdkvm_conv_cat_bias_act): channel counts in multiples of 64, same result bit for bit."""
    y = _conv_cat_operands("conv_cat_bias_act", x1, x2, x1.shape[2:] if x1.dim() == 4 else (), weight, bias, residual, packed)
    if packed is not None:
        tile |= CONV_PACKED_WEIGHTS
    n, c1, hh, ww = x1.shape
    _call("gdkvm_conv_cat_bias_act", x1.device, x1, x2, packed if packed is not None else weight, bias, residual, y,
          n, c1, x2.shape[1], hh, ww, y.shape[1], int(relu), tile, BF16)
    return y


def conv_upcat_bias_act(lo: torch.Tensor, x2: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
                        residual: Optional[torch.Tensor] = None, relu: bool = True,
                        packed: Optional[torch.Tensor] = None) -> torch.Tensor:
    """conv_cat_bias_act(upsample_bilinear(lo, x2.shape[2:]), x2, weight, ...) for an exact 2x enlargement, bit for bit, WITHOUT the
    enlarged tensor (gdkvm_conv_upcat_bias_act): lo channels_last bf16 [N,C1,H/2,W/2], x2 [N,C2,H,W] with H, W even and W <= 64;
    packed = conv3x3_pack_weights(weight) (made here when not given: the kernel reads only that form)."""
    size = (2 * lo.shape[2], 2 * lo.shape[3]) if lo.dim() == 4 else ()
    y = _conv_cat_operands("conv_upcat_bias_act", lo, x2, size, weight, bias, residual, packed)
    if packed is None:
        packed = conv3x3_pack_weights(weight)
    n, c1 = lo.shape[:2]
    _call("gdkvm_conv_upcat_bias_act", lo.device, lo, x2, packed, bias, residual, y,
          n, c1, x2.shape[1], size[0], size[1], y.shape[1], int(relu), CONV_PACKED_WEIGHTS, BF16)
    return y


def _upsample_cat_fwd(lo: torch.Tensor, skip: torch.Tensor) -> torch.Tensor:
    _channels_last("upsample_cat", lo, skip)
    if lo.dtype != torch.bfloat16 or skip.dtype != torch.bfloat16 or lo.shape[0] != skip.shape[0]:
        raise GdkvmError("upsample_cat: bf16 tensors with equal batch")
    n, c1, hl, wl = lo.shape
    _, c2, H, W = skip.shape
    out = torch.empty((n, c1 + c2, H, W), dtype=lo.dtype, device=lo.device, memory_format=torch.channels_last)
    _call("gdkvm_upsample_cat", lo.device, lo, skip, out, n, hl, wl, H, W, c1, c2, BF16)
    return out


def stem_conv_pool(xs: torch.Tensor, w_s2d: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """max_pool2d(relu(conv2d(xs, w_s2d, padding=2)[..., :Hs, :Ws] + bias), 3, 2, 1) in one kernel (gdkvm_stem_conv_pool):
    xs channels_last bf16 [N,16,Hs,Ws] (ops.stem_s2d), w_s2d channels_last bf16 [64,16,4,4], bias fp32 [64]."""
    if xs.dim() != 4 or not xs.is_cuda or xs.dtype != torch.bfloat16 or xs.shape[1] != 16 or \
            not xs.is_contiguous(memory_format=torch.channels_last):
        raise GdkvmError("stem_conv_pool needs a channels_last bf16 [N,16,Hs,Ws] device tensor (no CPU path)")
    if tuple(w_s2d.shape) != (64, 16, 4, 4) or w_s2d.dtype != torch.bfloat16 or not w_s2d.is_contiguous(memory_format=torch.channels_last):
        raise GdkvmError("stem_conv_pool: weight must be channels_last bf16 [64,16,4,4]")
    if bias.dtype != torch.float32 or bias.numel() != 64:
        raise GdkvmError("bias must be float32 [64]")
    n, _, hs, ws = xs.shape
    y = torch.empty((n, 64, (hs - 1) // 2 + 1, (ws - 1) // 2 + 1), dtype=xs.dtype, device=xs.device, memory_format=torch.channels_last)
    _call("gdkvm_stem_conv_pool", xs.device, xs, w_s2d, bias, y, n, hs, ws, BF16)
    return y


def stem_conv_pool_nchw(x: torch.Tensor, w_s2d: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """stem_conv_pool(stem_s2d(x, 16), w_s2d, bias) without the space-to-depth copy (gdkvm_stem_conv_pool_nchw): x contiguous NCHW bf16
    [N, C <= 4, H, W] with H, W even; bit-identical to the two-kernel form."""
    if x.dim() != 4 or not x.is_cuda or x.dtype != torch.bfloat16 or not x.is_contiguous() or x.shape[1] > 4 or x.shape[2] % 2 or x.shape[3] % 2:
        raise GdkvmError("stem_conv_pool_nchw needs a contiguous NCHW bf16 [N, C <= 4, H, W] device tensor with even H, W (no CPU path)")
    if tuple(w_s2d.shape) != (64, 16, 4, 4) or w_s2d.dtype != torch.bfloat16 or not w_s2d.is_contiguous(memory_format=torch.channels_last):
        raise GdkvmError("stem_conv_pool: weight must be channels_last bf16 [64,16,4,4]")
    if bias.dtype != torch.float32 or bias.numel() != 64:
        raise GdkvmError("bias must be float32 [64]")
    n, c, hh, ww = x.shape
    hs, ws = hh // 2, ww // 2
    y = torch.empty((n, 64, (hs - 1) // 2 + 1, (ws - 1) // 2 + 1), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    _call("gdkvm_stem_conv_pool_nchw", x.device, x, w_s2d, bias, y, n, c, hh, ww, BF16)
    return y


class _StemConvFunction(torch.autograd.Function):
    """The training stem's convolution (7x7 / stride 2 / pad 3, no bias, <= 4 input channels -> 64) on the hand-written stem kernel in its
    convolution-only form (gdkvm_stem_pack_s2d + gdkvm_stem_conv_nchw): bf16 NCHW frames in, channels_last bf16 out.  The input is the
    image (no data gradient); the weight gradient is gdkvm_stem_wgrad_nchw (stem_wgrad)."""

    @staticmethod
    def forward(ctx, x, weight):
        xb = x.detach().to(torch.bfloat16).contiguous()
        n, c, hh, ww = xb.shape
        w4 = torch.empty(64 * 256, dtype=torch.bfloat16, device=xb.device)
        y = torch.empty((n, 64, hh // 2, ww // 2), dtype=torch.bfloat16, device=xb.device, memory_format=torch.channels_last)
        wd = weight.detach()
        _call("gdkvm_stem_pack_s2d", xb.device, wd, w4, c, *wd.stride())
        _call("gdkvm_stem_conv_nchw", xb.device, xb, w4, y, n, c, hh, ww, BF16)
        ctx.save_for_backward(xb, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        xb, weight = ctx.saved_tensors
        dw = None
        if ctx.needs_input_grad[1]:
            dw = stem_wgrad(xb, dy, like=weight)
        return None, dw


def stem_wgrad(x: torch.Tensor, dy: torch.Tensor, like: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Weight gradient [64, C, 7, 7] fp32 of the stem convolution (7x7 / stride 2 / pad 3) for NCHW bf16 frames x [N, C <= 4, H, W] and
    dy [N, 64, H/2, W/2] (channels_last bf16), on gdkvm_stem_wgrad_nchw: fixed summation order, in the memory format of `like`."""
    xb = x.detach().to(torch.bfloat16).contiguous()
    dyb = _nhwc(dy.detach(), "stem_wgrad")
    if dyb.dtype != torch.bfloat16:
        dyb = dyb.to(torch.bfloat16)
    n, c, hh, ww = xb.shape
    if tuple(dyb.shape) != (n, 64, hh // 2, ww // 2):
        raise GdkvmError(f"stem_wgrad: dy {tuple(dyb.shape)} does not match x {tuple(xb.shape)}")
    dw = torch.empty_like(like, dtype=torch.float32) if like is not None else torch.empty((64, c, 7, 7), dtype=torch.float32, device=xb.device)
    ws = _workspace("gdkvm_stem_wgrad_workspace_bytes", xb.device, n, hh, ww)
    _call("gdkvm_stem_wgrad_nchw", xb.device, xb, dyb, dw, *dw.stride(), _Ws(ws), n, c, hh, ww, BF16)
    return dw


def stem_conv_served(x: torch.Tensor, conv) -> bool:
    w = conv.weight
    return (x.is_cuda and x.dim() == 4 and x.shape[1] <= 4 and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0 and conv.bias is None
            and tuple(w.shape) == (64, x.shape[1], 7, 7) and w.dtype == torch.float32 and conv.stride == (2, 2) and conv.padding == (3, 3)
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.padding_mode == "zeros"
            and (x.dtype == torch.bfloat16 or (torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16)))


def stem_conv(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """conv2d(x, weight, stride=2, padding=3) for the training stem (bf16 out, channels_last), differentiable in the weight."""
    return _StemConvFunction.apply(x, weight)


def upsample_cat_bwd(dout: torch.Tensor, lo_shape, skip_shape) -> Tuple[torch.Tensor, torch.Tensor]:
    """(d_lo, d_skip) of upsample_cat for d_out [N,C1+C2,H,W] channels_last bf16 (gdkvm_upsample_cat_bwd)."""
    dout = _nhwc(dout, "upsample_cat_bwd")
    if dout.dtype != torch.bfloat16:
        dout = dout.to(torch.bfloat16)
    n, c1, hl, wl = lo_shape
    _, c2, H, W = skip_shape
    if tuple(dout.shape) != (n, c1 + c2, H, W):
        raise GdkvmError(f"upsample_cat_bwd: d_out {tuple(dout.shape)} does not match {lo_shape} + {skip_shape}")
    dlo = torch.empty((n, c1, hl, wl), dtype=dout.dtype, device=dout.device, memory_format=torch.channels_last)
    dskip = torch.empty((n, c2, H, W), dtype=dout.dtype, device=dout.device, memory_format=torch.channels_last)
    _call("gdkvm_upsample_cat_bwd", dout.device, dout, dlo, dskip, n, hl, wl, H, W, c1, c2, BF16)
    return dlo, dskip


class _UpsampleCatFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lo, skip):
        ctx.shapes = (tuple(lo.shape), tuple(skip.shape))
        return _upsample_cat_fwd(lo, skip)

    @staticmethod
    def backward(ctx, dout):
        return upsample_cat_bwd(dout, *ctx.shapes)


def upsample_cat(lo: torch.Tensor, skip: torch.Tensor) -> torch.Tensor:
    """concat(bilinear_upsample(lo -> skip's H x W, align_corners=False), skip) along channels, both channels_last
    bf16 [N,C,h,w]; returns a channels_last [N,C1+C2,H,W] tensor (gdkvm_upsample_cat; differentiable:
    gdkvm_upsample_cat_bwd)."""
    if torch.is_grad_enabled() and (lo.requires_grad or skip.requires_grad):
        return _UpsampleCatFunction.apply(lo, skip)
    return _upsample_cat_fwd(lo, skip)


def _nhwc(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dim() != 4 or not t.is_cuda:
        raise GdkvmError(f"{what}: needs a [N,C,H,W] device tensor (no CPU path)")
    return t.contiguous(memory_format=torch.channels_last)


def bn_act_fwd(x, weight, bias, running_mean=None, running_var=None, residual=None, momentum: float = 0.1, eps: float = 1e-5,
               relu: bool = True):
    """Batch-statistics BatchNorm + optional residual add + optional ReLU on a channels_last tensor in three streaming
    passes (gdkvm_bn_fwd_train).  Updates running_mean / running_var in place.  Returns (y, stats) with stats fp32 [4, C] =
    (mean, 1/sqrt(var + eps), scale, shift)."""
    x = _nhwc(x, "bn_act_fwd")
    n, c, hh, ww = x.shape
    if residual is not None:
        residual = _nhwc(residual, "bn_act_fwd")
        if residual.shape != x.shape or residual.dtype != x.dtype:
            raise GdkvmError("bn_act_fwd: residual must match x (shape, dtype)")
    _f32_vectors("bn_act_fwd", c, weight, bias, running_mean, running_var)
    y = torch.empty_like(x)
    stats = torch.empty((4, c), dtype=torch.float32, device=x.device)
    ws = _workspace("gdkvm_bn_workspace_bytes", x.device, c)
    _call("gdkvm_bn_fwd_train", x.device, x, residual, weight, bias, running_mean, running_var, y, stats, _Ws(ws),
          n * hh * ww, c, float(eps), float(momentum), int(relu), _io_dtype(x))
    return y, stats


def bn_act_bwd(x, y, dy, weight, stats, relu: bool = True, want_dres: bool = False):
    """Backward of bn_act_fwd (gdkvm_bn_bwd): returns (dx, dres | None, dweight, dbias).  y = None with relu: the forward had
    no residual and the ReLU mask is recomputed from x (one tensor less to read)."""
    x, dy = _nhwc(x, "bn_act_bwd"), _nhwc(dy, "bn_act_bwd")
    if dy.dtype != x.dtype:
        dy = dy.to(x.dtype)
    if dy.shape != x.shape or (y is not None and y.shape != x.shape):
        raise GdkvmError("bn_act_bwd: shape mismatch")
    n, c, hh, ww = x.shape
    mode = 0 if not relu else (2 if y is None else 1)
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if (want_dres and relu) else None
    dgamma = torch.empty(c, dtype=torch.float32, device=x.device)
    dbeta = torch.empty_like(dgamma)
    ws = _workspace("gdkvm_bn_workspace_bytes", x.device, c)
    _call("gdkvm_bn_bwd", x.device, x, y if mode == 1 else None, dy, weight, stats, dx, dres, dgamma, dbeta, _Ws(ws),
          n * hh * ww, c, mode, _io_dtype(x))
    if want_dres and not relu:
        dres = dy                                           # no mask: the residual branch receives dy itself
    return dx, dres, dgamma, dbeta


class _BNActFunction(torch.autograd.Function):
    """y = act(BatchNorm_train(x) (+ residual)) with the HIP passes of csrc/bn.hip in both directions."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, running_mean, running_var, momentum, eps, relu):
        x = _nhwc(x, "bn_act")
        y, stats = bn_act_fwd(x, weight, bias, running_mean, running_var, residual, momentum, eps, relu)
        ctx.relu, ctx.has_res = relu, residual is not None
        ctx.save_for_backward(x, y if (relu and residual is not None) else None, weight, stats)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, weight, stats = ctx.saved_tensors
        dx, dres, dgamma, dbeta = bn_act_bwd(x, y, dy, weight, stats, ctx.relu, ctx.has_res and ctx.needs_input_grad[3])
        return dx, dgamma, dbeta, dres, None, None, None, None, None


def bn_act(x, weight, bias, running_mean=None, running_var=None, residual=None, momentum: float = 0.1, eps: float = 1e-5,
           relu: bool = True):
    """Differentiable fused BatchNorm(batch statistics) (+ residual) (+ ReLU); see bn_act_fwd."""
    return _BNActFunction.apply(x, weight, bias, residual, running_mean, running_var, momentum, eps, relu)


class _BNReluPoolFunction(torch.autograd.Function):
    """maxpool3x3s2(relu(BatchNorm_train(x))) as one op in both directions (gdkvm_bn_pool_fwd_train / gdkvm_bn_pool_bwd): the training
    stem's tail without the full-resolution activation or its gradient ever being written.  Same bits as bn_act + maxpool3x3s2."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps):
        x = _nhwc(x, "bn_relu_pool")
        n, c, hh, ww = x.shape
        ho, wo = (hh - 1) // 2 + 1, (ww - 1) // 2 + 1
        _f32_vectors("bn_relu_pool", c, weight, bias, running_mean, running_var)
        y = torch.empty((n, c, ho, wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
        idx = torch.empty((n, ho, wo, c), dtype=torch.uint8, device=x.device)
        stats = torch.empty((4, c), dtype=torch.float32, device=x.device)
        ws = _workspace("gdkvm_bn_workspace_bytes", x.device, c)
        _call("gdkvm_bn_pool_fwd_train", x.device, x, weight, bias, running_mean, running_var, y, idx, stats, _Ws(ws), n, hh, ww, c,
              float(eps), float(momentum), _io_dtype(x))
        ctx.save_for_backward(x, idx, weight, stats)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, idx, weight, stats = ctx.saved_tensors
        n, c, hh, ww = x.shape
        dy = _nhwc(dy, "bn_relu_pool backward")
        if dy.dtype != x.dtype:
            dy = dy.to(x.dtype)
        dx = torch.empty_like(x)
        dgamma = torch.empty(c, dtype=torch.float32, device=x.device)
        dbeta = torch.empty_like(dgamma)
        ws = _workspace("gdkvm_bn_workspace_bytes", x.device, c)
        _call("gdkvm_bn_pool_bwd", x.device, x, dy, idx, weight, stats, dx, dgamma, dbeta, _Ws(ws), n, hh, ww, c, _io_dtype(x))
        return dx, dgamma, dbeta, None, None, None, None


def bn_relu_pool_served(x: torch.Tensor) -> bool:
    return (x.is_cuda and x.dim() == 4 and x.dtype == torch.bfloat16 and x.shape[1] % 8 == 0 and x.shape[1] // 8 <= 256
            and x.shape[0] * x.shape[2] * x.shape[3] < (1 << 22))


def bn_relu_pool(x, weight, bias, running_mean=None, running_var=None, momentum: float = 0.1, eps: float = 1e-5):
    """maxpool3x3s2(bn_act(x, ..., relu=True)) as one differentiable op (the training stem's tail); bf16 channels_last."""
    return _BNReluPoolFunction.apply(x, weight, bias, running_mean, running_var, momentum, eps)


class _MaxPoolFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _nhwc(x, "maxpool3x3s2")
        n, c, hh, ww = x.shape
        ho, wo = (hh - 1) // 2 + 1, (ww - 1) // 2 + 1
        y = torch.empty((n, c, ho, wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
        idx = torch.empty((n, ho, wo, c), dtype=torch.uint8, device=x.device)
        _call("gdkvm_maxpool_fwd", x.device, x, y, idx, n, hh, ww, c, _io_dtype(x))
        ctx.save_for_backward(idx)
        ctx.in_shape = (n, c, hh, ww)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        n, c, hh, ww = ctx.in_shape
        dy = _nhwc(dy, "maxpool3x3s2 backward")
        dx = torch.empty((n, c, hh, ww), dtype=dy.dtype, device=dy.device, memory_format=torch.channels_last)
        _call("gdkvm_maxpool_bwd", dy.device, dy, idx, dx, n, hh, ww, c, _io_dtype(dy))
        return dx


def maxpool3x3s2(x: torch.Tensor) -> torch.Tensor:
    """max_pool2d(x, 3, 2, 1) on a channels_last tensor, differentiable (gdkvm_maxpool_fwd / _bwd: the backward is a gather
    from the recorded winning taps, PyTorch's tie rule)."""
    return _MaxPoolFunction.apply(x)


def gemm_nt(a: torch.Tensor, bt: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """C [M,N] = a [M,K] @ bt [N,K]^T (+ bias [N], fp32) on the hand-written MFMA kernel (gdkvm_gemm_nt); a, bt share one dtype
    (bf16 or fp32), C comes back in it, accumulation is fp32."""
    if a.dim() != 2 or bt.dim() != 2 or a.shape[1] != bt.shape[1] or a.dtype != bt.dtype:
        raise GdkvmError(f"gemm_nt: a [M,K] and bt [N,K] of one dtype, got {tuple(a.shape)} {a.dtype} / {tuple(bt.shape)} {bt.dtype}")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != bt.shape[0]):
        raise GdkvmError("gemm_nt: bias must be float32 [N]")
    kq = 32 if a.dtype == torch.bfloat16 else 16
    if a.shape[1] % kq:                                     # an odd contraction length: zero columns up to the MFMA's k step
        pad = kq - a.shape[1] % kq
        a, bt = torch.nn.functional.pad(a, (0, pad)), torch.nn.functional.pad(bt, (0, pad))
    dev = _dev(a, bt, bias)
    M, K = a.shape
    N = bt.shape[0]
    c = torch.empty((M, N), dtype=a.dtype, device=dev)
    _call("gdkvm_gemm_nt", dev, a, bt, bias, c, M, N, K, _io_dtype(a))
    return c


def wgrad(dy2d: torch.Tensor, x2d: torch.Tensor, colsum: bool = False):
    """dW [M,N] (fp32) = dy^T x for token-major operands dy [K,M], x [K,N] with K (the tokens of the batch) >> M, N: the
    reduction over the tokens is split over workgroups into fp32 partial tiles and summed in a fixed order (gdkvm_gemm_tn);
    the sum never passes through bf16.  colsum=True: (dW, db) with db [M] (fp32) = the column sums of dy -- the bias gradient --
    from the same launch (gdkvm_gemm_tn_colsum)."""
    if dy2d.dim() != 2 or x2d.dim() != 2 or dy2d.shape[0] != x2d.shape[0]:
        raise GdkvmError("wgrad: dy [K,M] and x [K,N] with equal K")
    if dy2d.dtype != x2d.dtype:
        x2d = x2d.to(dy2d.dtype)
    dy2d, x2d = dy2d.contiguous(), x2d.contiguous()
    dev = _dev(dy2d, x2d)
    K, M = dy2d.shape
    N = x2d.shape[1]
    c = torch.empty((M, N), dtype=torch.float32, device=dev)
    name = "gdkvm_gemm_tn_colsum" if colsum else "gdkvm_gemm_tn"
    outs = (c, torch.empty(M, dtype=torch.float32, device=dev)) if colsum else (c,)
    ws = _workspace(name + "_workspace_bytes", dev, K, M, N)
    _call(name, dev, dy2d, x2d, *outs, _Ws(ws), K, M, N, _io_dtype(dy2d))
    return outs if colsum else c


class _TokenLinear(torch.autograd.Function):
    """y = x W^T + b on token rows [K, Cin] (the 1x1 projections), forward and backward on the hand-written products:
    gdkvm_gemm_nt with the bias in its epilogue; dX = dY W as gdkvm_gemm_nt on the weight with its input index leading; dW
    through wgrad (gdkvm_gemm_tn)."""

    @staticmethod
    def forward(ctx, x2d, weight, bias):
        w = weight.to(x2d.dtype).contiguous()
        x2d = x2d.contiguous()
        ctx.save_for_backward(x2d, w)
        ctx.has_bias, ctx.wdtype = bias is not None, weight.dtype
        return gemm_nt(x2d, w, None if bias is None else bias.detach().float().contiguous())

    @staticmethod
    def backward(ctx, dy):
        x2d, w = ctx.saved_tensors
        dy = dy.contiguous()
        dx = gemm_nt(dy, w.t().contiguous()) if ctx.needs_input_grad[0] else None
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        dw = db = None
        if ctx.needs_input_grad[1] and want_b and dy.is_cuda:
            dw, db = wgrad(dy, x2d, colsum=True)            # the bias gradient rides on the weight gradient's launch (one more MFMA per step)
            dw, db = dw.to(ctx.wdtype), db.to(ctx.wdtype)
        else:
            if ctx.needs_input_grad[1]:
                dw = wgrad(dy, x2d).to(ctx.wdtype)
            if want_b:                                      # (column sums with fp32 accumulation straight from the rows)
                db = dy.sum(0, dtype=torch.float32).to(ctx.wdtype)
        return dx, dw, db


def token_linear(x2d: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    return _TokenLinear.apply(x2d, weight, bias)


class _TokenProjections(torch.autograd.Function):
    """Several 1x1 projections of the SAME token rows (key, query, value, write gate) as ONE product against their stacked weights, forward
    and backward: y_i = x W_i^T + b_i.  As four _TokenLinear calls a training step spent ~55 launches on them -- per projection a weight cast, the
    product, a transposed weight copy, the data-gradient product, an add into the feature's gradient, the split-K weight gradient and its
    sum, plus zero-padding of the one-row gate projection both ways; stacked it is: cat + cast of the weights, cat of the biases, one
    gdkvm_gemm_nt, one copy per output (contiguous rows for the scan kernels) -- and backward one cat of the incoming gradients, one
    transposed weight copy, one gdkvm_gemm_nt for dX and one gdkvm_gemm_tn_colsum for every dW and db (returned as row slices of its result).
    The stacked width is padded with zero rows to a multiple of 32 (the MFMA's k step in the dX product)."""

    @staticmethod
    def forward(ctx, x2d, *wb):
        ws, bs = wb[0::2], wb[1::2]
        x2d = x2d.contiguous()
        widths = [int(w.shape[0]) for w in ws]
        total = sum(widths)
        padded = (total + 31) // 32 * 32
        cin = x2d.shape[1]
        parts = [w.detach().reshape(w.shape[0], cin) for w in ws]
        if padded > total:
            parts.append(torch.zeros((padded - total, cin), dtype=parts[0].dtype, device=x2d.device))
        w_all = torch.cat(parts, 0).to(x2d.dtype)
        b_parts = [(b.detach().float() if b is not None else torch.zeros(n, dtype=torch.float32, device=x2d.device)) for b, n in zip(bs, widths)]
        if padded > total:
            b_parts.append(torch.zeros(padded - total, dtype=torch.float32, device=x2d.device))
        y = gemm_nt(x2d, w_all, torch.cat(b_parts, 0))
        ctx.save_for_backward(x2d, w_all)
        ctx.widths, ctx.padded = widths, padded
        ctx.meta = [(w.dtype, tuple(w.shape), b is not None, None if b is None else b.dtype) for w, b in zip(ws, bs)]
        outs, o = [], 0
        for n in widths:
            outs.append(y[:, o:o + n].contiguous())
            o += n
        return tuple(outs)

    @staticmethod
    def backward(ctx, *dys):
        x2d, w_all = ctx.saved_tensors
        widths, padded = ctx.widths, ctx.padded
        total = sum(widths)
        parts = [dy.to(x2d.dtype) if dy is not None else torch.zeros((x2d.shape[0], n), dtype=x2d.dtype, device=x2d.device) for dy, n in zip(dys, widths)]
        if padded > total:
            parts.append(torch.zeros((x2d.shape[0], padded - total), dtype=x2d.dtype, device=x2d.device))
        dy_all = torch.cat(parts, 1)
        dx = gemm_nt(dy_all, w_all.t().contiguous()) if ctx.needs_input_grad[0] else None
        grads = [dx]
        need_w = any(ctx.needs_input_grad[1 + 2 * i] for i in range(len(widths)))
        need_b = any(ctx.needs_input_grad[2 + 2 * i] and ctx.meta[i][2] for i in range(len(widths)))
        dw_all = db_all = None
        if need_w or need_b:
            dw_all, db_all = wgrad(dy_all, x2d, colsum=True)
        o = 0
        for i, n in enumerate(widths):
            wdt, wshape, has_b, bdt = ctx.meta[i]
            dw = dw_all[o:o + n].reshape(wshape).to(wdt) if ctx.needs_input_grad[1 + 2 * i] else None
            db = db_all[o:o + n].to(bdt) if (has_b and ctx.needs_input_grad[2 + 2 * i]) else None
            grads += [dw, db]
            o += n
        return tuple(grads)


def token_projections(x2d: torch.Tensor, layers) -> Tuple[torch.Tensor, ...]:
    """[conv(x) for conv in layers] for 1x1 convolutions (or Linear layers) applied to token rows x2d [rows, Cin]: one stacked product
    forward, two backward (_TokenProjections).  Each result is a contiguous [rows, out_channels] tensor in x2d's dtype."""
    args = []
    for m in layers:
        args += [m.weight, m.bias]
    return _TokenProjections.apply(x2d, *args)


class _SegLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, target, H, W, dice_weight, eps):
        if z.dim() != 4 or not z.is_cuda or target.dim() != 3 or target.shape[0] != z.shape[0]:
            raise GdkvmError("seg_loss: logits [images,C,h,w] and labels [images,H,W] on the device (no CPU path)")
        if target.dtype not in (torch.int64, torch.uint8) or tuple(target.shape[1:]) != (H, W):
            raise GdkvmError("seg_loss: labels must be int64 or uint8 [images,H,W]")
        z, target = z.contiguous(), target.contiguous()
        ni, c, h, w = z.shape
        out = torch.empty(3, dtype=torch.float32, device=z.device)
        ws = _workspace("gdkvm_seg_loss_workspace_bytes", z.device, c)
        tb = 8 if target.dtype == torch.int64 else 1
        _call("gdkvm_seg_loss_fwd", z.device, z, target, out, _Ws(ws), ni, c, h, w, H, W, float(dice_weight), float(eps), _io_dtype(z), tb)
        ctx.save_for_backward(z, target, ws)
        ctx.dims = (ni, c, h, w, H, W, tb)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        z, target, ws = ctx.saved_tensors
        ni, c, h, w, H, W, tb = ctx.dims
        g = g.to(torch.float32).reshape(1).contiguous()
        dz = torch.empty_like(z)
        _call("gdkvm_seg_loss_bwd", z.device, z, target, _Ws(ws), g, dz, ni, c, h, w, H, W, _io_dtype(z), tb)
        return dz, None, None, None, None, None


def seg_loss(lowres_logits: torch.Tensor, target: torch.Tensor, dice_weight: float = 1.0, eps: float = 1.0) -> torch.Tensor:
    """Cross-entropy + soft Dice of bilinear_upsample(lowres_logits -> target's H x W) against integer labels, without the
    full-resolution logits (gdkvm_seg_loss_fwd / _bwd).  lowres_logits [images,C,h,w], target [images,H,W]; scalar loss."""
    return _SegLossFunction.apply(lowres_logits, target, target.shape[-2], target.shape[-1], dice_weight, eps)


SIGNED_DISTANCE_MAX_CLASSES = 32


def _class_mask(what: str, num_classes: int, classes, default_from: int) -> int:
    """Bit c = class c takes part.  classes None: every class from `default_from` on; otherwise distinct integers in 0..num_classes - 1."""
    if classes is None:
        return ((1 << int(num_classes)) - 1) & ~((1 << default_from) - 1)
    cl = list(classes)
    if any(isinstance(c, bool) or int(c) != c or not 0 <= int(c) < num_classes for c in cl) or len({int(c) for c in cl}) != len(cl):
        raise GdkvmError(f"{what}: classes = {cl} must be distinct integers in 0..{num_classes - 1}")
    mask = 0
    for c in cl:
        mask |= 1 << int(c)
    return mask


def _labels_u8(target: torch.Tensor, num_classes: int) -> torch.Tensor:
    """uint8 labels for the per-frame mask kernels: uint8 passes, int64 has everything outside [0, num_classes) mapped to 255 before the cast
    (a plain cast would fold 256 onto class 0)."""
    if target.dtype == torch.uint8:
        return target
    return torch.where((target < 0) | (target >= num_classes), 255, target).to(torch.uint8)


def signed_distance(target: torch.Tensor, num_classes: int, classes=None, _mask: Optional[int] = None) -> torch.Tensor:
    """gdkvm_signed_distance: per frame of target [..., H, W] (uint8, or int64 labels) and class c < num_classes the signed squared Euclidean
    distance of every pixel to the class's contour -- + the squared distance to the nearest pixel of the class outside it, - the squared
    distance to the nearest pixel outside the class inside it, 0 everywhere when the frame has no pixel of the class or no other (definition:
    include/gdkvm.h; every output is an exact integer).  Returns int32 [..., num_classes, H, W]; `classes` (default: all) names the classes that
    are computed, the planes of the others are zero.  The operand sd2 of seg_loss_boundary."""
    if target.dtype not in (torch.uint8, torch.int64) or target.dim() < 2:
        raise GdkvmError(f"signed_distance: target must be uint8 or int64 [..., H, W], got {target.dtype} {tuple(target.shape)}")
    C = int(num_classes)
    if not 1 <= C <= SIGNED_DISTANCE_MAX_CLASSES:
        raise GdkvmError(f"signed_distance: num_classes = {num_classes} outside 1..{SIGNED_DISTANCE_MAX_CLASSES}")
    mask = _class_mask("signed_distance", C, classes, 0) if _mask is None else _mask
    dev = _dev(target)
    t8 = _labels_u8(target, C)
    lead, frames, H, W = _mask_frames("signed_distance", t8, 0)
    sd2 = torch.empty(lead + (C, H, W), dtype=torch.int32, device=dev)
    ws = _workspace("gdkvm_signed_distance_workspace_bytes", dev, frames, C, H, W, floor=16)
    _call("gdkvm_signed_distance", dev, t8, sd2, _Ws(ws), frames, C, H, W, mask)
    return sd2


class _SegLossBoundaryFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, target, sd2, out, H, W, dice_weight, eps, boundary_weight, mask):
        if z.dim() != 4 or not z.is_cuda or target.dim() != 3 or target.shape[0] != z.shape[0]:
            raise GdkvmError("seg_loss_boundary: logits [images,C,h,w] and labels [images,H,W] on the device (no CPU path)")
        if target.dtype not in (torch.int64, torch.uint8) or tuple(target.shape[1:]) != (H, W):
            raise GdkvmError("seg_loss_boundary: labels must be int64 or uint8 [images,H,W]")
        if not (math.isfinite(float(boundary_weight)) and float(boundary_weight) >= 0.0):
            raise GdkvmError(f"seg_loss_boundary: boundary_weight = {boundary_weight} must be finite and >= 0")
        z, target = z.contiguous(), target.contiguous()
        ni, c, h, w = z.shape
        if sd2 is None:
            sd2 = signed_distance(target, c, _mask=mask)
        elif sd2.dtype != torch.int32 or tuple(sd2.shape) != (ni, c, H, W) or sd2.device != z.device or not sd2.is_contiguous():
            raise GdkvmError(f"seg_loss_boundary: sd2 must be contiguous int32 {(ni, c, H, W)} on the logits' device (ops.signed_distance)")
        ws = _workspace("gdkvm_seg_loss_boundary_workspace_bytes", z.device, c)
        tb = 8 if target.dtype == torch.int64 else 1
        _call("gdkvm_seg_loss_boundary_fwd", z.device, z, target, sd2, out, _Ws(ws), ni, c, h, w, H, W, float(dice_weight), float(eps),
              float(boundary_weight), mask, _io_dtype(z), tb)
        ctx.save_for_backward(z, target, sd2, ws)
        ctx.dims = (ni, c, h, w, H, W, tb, mask)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        z, target, sd2, ws = ctx.saved_tensors
        ni, c, h, w, H, W, tb, mask = ctx.dims
        g = g.to(torch.float32).reshape(1).contiguous()
        dz = torch.empty_like(z)
        _call("gdkvm_seg_loss_boundary_bwd", z.device, z, target, sd2, _Ws(ws), g, dz, ni, c, h, w, H, W, mask, _io_dtype(z), tb)
        return (dz,) + (None,) * 9


def seg_loss_boundary(lowres_logits: torch.Tensor, target: torch.Tensor, dice_weight: float = 1.0, eps: float = 1.0,
                      boundary_weight: float = 0.0, classes=None, sd2: Optional[torch.Tensor] = None, terms: bool = False):
    """seg_loss plus boundary_weight * the boundary loss of Kervadec et al. (gdkvm_seg_loss_boundary_fwd / _bwd; definition: include/gdkvm.h):
    the mean over the labelled pixels of sum_{c in classes} softmax_c * signed distance to the contour of class c in `target`.  `classes`
    default: every class but 0; the term is not divided by their number.  sd2: ops.signed_distance(target, C) when the caller has it already
    (planes outside `classes` are not read); built here otherwise, and kept for the backward either way.  Scalar loss; terms=True: (loss,
    float32 [4] = loss, CE, Dice term, L_B, detached)."""
    mask = _class_mask("seg_loss_boundary", lowres_logits.shape[1], classes, 1)
    out = torch.empty(4, dtype=torch.float32, device=lowres_logits.device)          # (written by the forward; never part of the autograd graph)
    loss = _SegLossBoundaryFunction.apply(lowres_logits, target, sd2, out, target.shape[-2], target.shape[-1], dice_weight, eps,
                                          boundary_weight, mask)
    return (loss, out) if terms else loss


def dice_from_counts(counts: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """Dice_c = (2|AnB| + eps) / (|A| + |B| + eps) from the integer counts of argmax_dice."""
    c = counts.to(torch.float64)
    return (2.0 * c[..., 0] + eps) / (c[..., 1] + c[..., 2] + eps)


def iou_from_counts(counts: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """IoU_c = (|AnB| + eps) / (|A| + |B| - |AnB| + eps) from the same counts (dice_from_counts' eps convention: an absent class scores 1)."""
    c = counts.to(torch.float64)
    return (c[..., 0] + eps) / (c[..., 1] + c[..., 2] - c[..., 0] + eps)


LV_MAX_SIDE, LV_MAX_DISKS = 1024, 64


def lv_measure(mask: torch.Tensor, cls: int = 1, disks: int = 20):
    """gdkvm_lv_measure: per frame of mask [..., H, W] uint8 the pixel moments of class `cls`, its long axis, the overlap-weighted areas of
    `disks` disks along it and the single-plane method-of-disks volume (definition: include/gdkvm.h; integer-exact up to the disk areas).
    Returns (stats int64 [..., 12] = n sx sy sxx sxy syy Ux Uy tmin tmax Lt 0, disks int64 [..., D], geom float64 [..., 4] = L V cx cy);
    lengths in pixels of the mask's grid, V in pixel^3.  The mask may start at any byte address."""
    return _lv_measure("gdkvm_lv_measure", mask, None, cls, disks)


SPACING_UM_MAX = 4095           # a pixel spacing is (row_um, col_um), integers in 1..SPACING_UM_MAX micrometres
SURFACE_MM_LDS_PIXELS = 18432   # GDKVM_SURFACE_MM_LDS_PIXELS: frames of up to this many pixels need no workspace in surface_distance_mm


def _spacing_frames(what: str, spacing_um: torch.Tensor, lead, dev) -> torch.Tensor:
    """spacing_um int32 [..., 2] broadcast over the mask's leading shape `lead` -> a contiguous int32 [*lead, 2] on `dev`.  A CPU tensor is
    range-checked here and copied; a device tensor is trusted (the kernels answer an out-of-range frame with -1 everywhere)."""
    if not isinstance(spacing_um, torch.Tensor) or spacing_um.dtype != torch.int32 or spacing_um.dim() < 1 or spacing_um.shape[-1] != 2:
        raise GdkvmError(f"{what}: spacing_um must be an int32 tensor [..., 2] = (row_um, col_um), got "
                         f"{getattr(spacing_um, 'dtype', type(spacing_um))} {tuple(getattr(spacing_um, 'shape', ()))}")
    if not spacing_um.is_cuda:
        if spacing_um.numel() and (int(spacing_um.min()) < 1 or int(spacing_um.max()) > SPACING_UM_MAX):
            raise GdkvmError(f"{what}: spacing_um outside 1..{SPACING_UM_MAX} micrometres")
        spacing_um = spacing_um.to(dev)
    elif spacing_um.device != dev:
        raise GdkvmError("tensors on different devices")
    try:
        return spacing_um.expand(tuple(lead) + (2,)).contiguous()
    except RuntimeError:
        raise GdkvmError(f"{what}: spacing_um {tuple(spacing_um.shape)} does not broadcast over the mask's leading shape {tuple(lead)}") from None


def lv_measure_mm(mask: torch.Tensor, spacing_um: torch.Tensor, cls: int = 1, disks: int = 20):
    """gdkvm_lv_measure_mm: lv_measure with a pixel spacing -- spacing_um int32 [..., 2] = (row_um, col_um) micrometres per pixel, broadcast
    over mask's leading dimensions ([B, 1, 2] against [B, T, H, W]); the long axis is found in the physical plane (definition:
    include/gdkvm.h).  Returns (stats int64 [..., 12] = n sx sy sxx sxy syy Vx Vy tmin tmax Lt E, disks int64 [..., D], geom float64
    [..., 6] = L in mm, V in mL, cx, cy in mm, k = um per pixel extent along the axis, area in mm^2).  A frame whose spacing (a device
    tensor's: a host tensor is refused) is outside 1..4095 holds -1 everywhere."""
    return _lv_measure("gdkvm_lv_measure_mm", mask, spacing_um, cls, disks)


def _lv_measure(entry: str, mask, spacing_um, cls, disks):
    """lv_measure (spacing_um None) and lv_measure_mm behind their entry point: the spacing in front of the outputs, geom 4 or 6 wide"""
    what = entry[len("gdkvm_"):]
    lead, frames, H, W = _mask_frames(what, mask, cls)
    if not 1 <= int(disks) <= LV_MAX_DISKS:
        raise GdkvmError(f"{what}: disks = {disks} outside 1..{LV_MAX_DISKS}")
    dev = _dev(mask)
    sp = () if spacing_um is None else (_spacing_frames(what, spacing_um, lead, dev),)
    stats = torch.empty(lead + (12,), dtype=torch.int64, device=dev)
    dk = torch.empty(lead + (int(disks),), dtype=torch.int64, device=dev)
    geom = torch.empty(lead + (6 if sp else 4,), dtype=torch.float64, device=dev)
    _call(entry, dev, mask, *sp, stats, dk, geom, frames, H, W, int(cls), int(disks))
    return stats, dk, geom


def lv_ef(vol: torch.Tensor, npix: torch.Tensor, pick_vol: Optional[torch.Tensor] = None, pick_npix: Optional[torch.Tensor] = None,
          min_pixels: int = 1):
    """gdkvm_lv_ef: per clip the end-diastolic / end-systolic frames and the ejection fraction from vol float64 [B, T] and npix int64 [B, T]
    (lv_measure's geom[..., 1] and stats[..., 0]; non-contiguous views are copied).  Frames with fewer than `min_pixels` pixels are not
    candidates; with pick_vol / pick_npix (both or neither, same shapes) ED / ES are chosen on THOSE -- the prediction's volumes at the
    target's frames.  Returns (ed_es_nvalid int32 [B, 3], edv_esv_ef float64 [B, 3]); fewer than two valid frames: ed = es = -1, EF = 0."""
    if (pick_vol is None) != (pick_npix is None):
        raise GdkvmError("lv_ef: pick_vol and pick_npix go together")
    if vol.dim() != 2 or vol.shape[1] < 1:
        raise GdkvmError(f"lv_ef: vol must be [B, T] with T >= 1, got {tuple(vol.shape)}")
    for name, t, dt in (("vol", vol, torch.float64), ("npix", npix, torch.int64), ("pick_vol", pick_vol, torch.float64),
                        ("pick_npix", pick_npix, torch.int64)):
        if t is not None and (t.dtype != dt or tuple(t.shape) != tuple(vol.shape)):
            raise GdkvmError(f"lv_ef: {name} must be {dt} {tuple(vol.shape)}, got {t.dtype} {tuple(t.shape)}")
    vol, npix, pick_vol, pick_npix = (None if t is None else t.contiguous() for t in (vol, npix, pick_vol, pick_npix))
    dev = _dev(vol, npix, pick_vol, pick_npix)
    B, T = vol.shape
    idx = torch.empty((B, 3), dtype=torch.int32, device=dev)
    val = torch.empty((B, 3), dtype=torch.float64, device=dev)
    _call("gdkvm_lv_ef", dev, vol, npix, pick_vol, pick_npix, idx, val, B, T, int(min_pixels))
    return idx, val


def ef_summary(pred_ef: torch.Tensor, ref_ef: torch.Tensor, ok: torch.Tensor) -> torch.Tensor:
    """The eight running sums of an EF comparison over the clips where `ok`: count, sum e, sum |e|, sum p, sum g, sum p^2, sum g^2, sum p g
    (e = p - g; float64 [8], on the inputs' device).  Sums of batches and of ranks add, so a multi-GPU evaluation needs one small
    all_reduce, like the Dice counts; ef_stats turns them into MAE, bias and Pearson r."""
    k = ok.to(torch.float64)
    p, g = pred_ef.to(torch.float64) * k, ref_ef.to(torch.float64) * k
    e = p - g
    return torch.stack([k.sum(), e.sum(), e.abs().sum(), p.sum(), g.sum(), (p * p).sum(), (g * g).sum(), (p * g).sum()])


def ef_stats(sums) -> dict:
    """{clips_with_ef, ef_mae, ef_bias, ef_pearson_r, mean_ref_ef, mean_pred_ef} from ef_summary's sums (host numbers; r is 0 when either
    side has no variance or fewer than two clips count)."""
    n, se, sae, sp, sg, spp, sgg, spg = (float(v) for v in sums)
    if n < 1:
        return {"clips_with_ef": 0, "ef_mae": 0.0, "ef_bias": 0.0, "ef_pearson_r": 0.0, "mean_ref_ef": 0.0, "mean_pred_ef": 0.0}
    vp, vg, cov = n * spp - sp * sp, n * sgg - sg * sg, n * spg - sp * sg
    r = cov / (vp * vg) ** 0.5 if n >= 2 and vp > 0 and vg > 0 else 0.0
    return {"clips_with_ef": int(n), "ef_mae": sae / n, "ef_bias": se / n, "ef_pearson_r": r, "mean_ref_ef": sg / n, "mean_pred_ef": sp / n}


LV_BEATS_MAX_T, LV_BEATS_MAX_BEATS = 4096, 64


def lv_beats(area: torch.Tensor, vol: torch.Tensor, length: Optional[torch.Tensor] = None, max_beats: int = 16, distance: int = 20,
             prominence_permille: int = 500, min_pixels: int = 1):
    """gdkvm_lv_beats: per clip the heart beats of the curves area int64 [B, T] and vol float64 [B, T] (lv_measure's stats[..., 0] and
    geom[..., 1]; non-contiguous views are copied): the end-systoles are the strict local minima of `area` that scipy.signal.find_peaks(-area,
    distance=distance, prominence=prominence_permille / 1000 * range) keeps, each beat's end-diastole the largest area in front of its
    end-systole, one EF per beat (definition: include/gdkvm.h; integer-exact up to the EF).  length int32 [B] on the same device: only the
    frames 0 .. length[b] - 1 of clip b count (None: all T).  Returns (beats int32 [B, max_beats, 2] = ed, es or -1, beat_val float64
    [B, max_beats, 3] = EDV, ESV, EF, info int32 [B, 4] = n_beats, end-systoles, frames below min_pixels, last - first end-systole, summ
    float64 [B, 4] = mean, smallest, largest beat EF, mean cycle in frames)."""
    if area.dim() != 2 or not 1 <= area.shape[1] <= LV_BEATS_MAX_T:
        raise GdkvmError(f"lv_beats: area must be [B, T] with T in 1..{LV_BEATS_MAX_T}, got {tuple(area.shape)}")
    for name, t, dt in (("area", area, torch.int64), ("vol", vol, torch.float64)):
        if t.dtype != dt or tuple(t.shape) != tuple(area.shape):
            raise GdkvmError(f"lv_beats: {name} must be {dt} {tuple(area.shape)}, got {t.dtype} {tuple(t.shape)}")
    B, T = area.shape
    if length is not None and (length.dtype != torch.int32 or tuple(length.shape) != (B,)):
        raise GdkvmError(f"lv_beats: length must be int32 [{B}], got {length.dtype} {tuple(length.shape)}")
    if not 1 <= int(max_beats) <= LV_BEATS_MAX_BEATS:
        raise GdkvmError(f"lv_beats: max_beats = {max_beats} outside 1..{LV_BEATS_MAX_BEATS}")
    if not 1 <= int(distance) <= LV_BEATS_MAX_T:
        raise GdkvmError(f"lv_beats: distance = {distance} outside 1..{LV_BEATS_MAX_T}")
    if not 0 <= int(prominence_permille) <= 1000:
        raise GdkvmError(f"lv_beats: prominence_permille = {prominence_permille} outside 0..1000")
    area, vol, length = (None if t is None else t.contiguous() for t in (area, vol, length))
    dev = _dev(area, vol, length)
    beats = torch.empty((B, int(max_beats), 2), dtype=torch.int32, device=dev)
    beat_val = torch.empty((B, int(max_beats), 3), dtype=torch.float64, device=dev)
    info = torch.empty((B, 4), dtype=torch.int32, device=dev)
    summ = torch.empty((B, 4), dtype=torch.float64, device=dev)
    _call("gdkvm_lv_beats", dev, area, vol, length, beats, beat_val, info, summ, B, T, int(max_beats), int(distance), int(prominence_permille),
          int(min_pixels))
    return beats, beat_val, info, summ


def lv_biplane(stats: torch.Tensor, disks: torch.Tensor, geom: torch.Tensor, spacing_um: torch.Tensor, pairs: torch.Tensor):
    """gdkvm_lv_biplane: the bi-plane Simpson volume of every frame from the records of two views.  stats int64 [C, T, 12], disks int64
    [C, T, D] and geom float64 [C, T, 6] are lv_measure_mm's outputs for C clips of T frames (non-contiguous views are copied), spacing_um the
    int32 [..., 2] that call was given, broadcast over [C, T] as there; pairs a HOST int32 [P, 2] tensor whose rows are the clip indices of
    view a and view b (eval.py: the 2CH and the 4CH clip of a patient, gdkvm_amd.data.view_pair_table) -- it is range-checked against C here,
    before anything is copied, and a device tensor is refused.  Disk j of both views must count from the same end of the ventricle
    (definition and the assumption: include/gdkvm.h).  Returns (out float64 [P, T, 3] = V in mL, L in mm, the long axes' mismatch (L - the
    shorter) / L; npix int64 [P, T] = the smaller view's pixels, 0 where either view is empty or has a -1 record, and then out is 0 too);
    lv_ef(out[..., 0], npix) gives ED / ES / EF per pair."""
    for name, t, dt, last in (("stats", stats, torch.int64, 12), ("disks", disks, torch.int64, None), ("geom", geom, torch.float64, 6)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 3 or (last is not None and t.shape[2] != last):
            raise GdkvmError(f"lv_biplane: {name} must be {dt} [C, T, {last or 'D'}], got {getattr(t, 'dtype', type(t))} "
                             f"{tuple(getattr(t, 'shape', ()))}")
    C, T = int(stats.shape[0]), int(stats.shape[1])
    D = int(disks.shape[2])
    if tuple(disks.shape[:2]) != (C, T) or tuple(geom.shape[:2]) != (C, T):
        raise GdkvmError(f"lv_biplane: stats {tuple(stats.shape)}, disks {tuple(disks.shape)} and geom {tuple(geom.shape)} are not records of "
                         "the same [C, T] frames")
    if not 1 <= D <= LV_MAX_DISKS:
        raise GdkvmError(f"lv_biplane: disks = {D} outside 1..{LV_MAX_DISKS}")
    if not isinstance(pairs, torch.Tensor) or pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 2:
        raise GdkvmError(f"lv_biplane: pairs must be an int32 tensor [P, 2] = (clip of view a, clip of view b), got "
                         f"{getattr(pairs, 'dtype', type(pairs))} {tuple(getattr(pairs, 'shape', ()))}")
    if pairs.device.type != "cpu":
        raise GdkvmError("lv_biplane: pairs must be a host tensor (it is range-checked before it is copied)")
    if pairs.numel() and (int(pairs.min()) < 0 or int(pairs.max()) >= C):
        raise GdkvmError(f"lv_biplane: a pair names a clip outside 0..{C - 1}")
    stats, disks, geom = stats.contiguous(), disks.contiguous(), geom.contiguous()
    dev = _dev(stats, disks, geom)
    sp = _spacing_frames("lv_biplane", spacing_um, (C, T), dev)
    P = int(pairs.shape[0])
    pr = pairs.contiguous().to(dev)
    out = torch.empty((P, T, 3), dtype=torch.float64, device=dev)
    npix = torch.empty((P, T), dtype=torch.int64, device=dev)
    _call("gdkvm_lv_biplane", dev, stats, disks, geom, sp, pr, out, npix, C, T, D, P)
    return out, npix


LV_CONTOUR_BAND_ROWS, LV_CONTOUR_WORD_BITS = 64, 64      # GDKVM_LV_CONTOUR_BAND_ROWS, GDKVM_LV_CONTOUR_WORD_BITS
LV_CONTOUR_MAX_BYTE = 31                                 # cls and the members of the sets are bytes in 0..31

# (dy, dx) of a class pixel's 8 neighbours under the direction their pair counts for: E, S, SE, SW
_CONTOUR_NEIGHBOURS = (((0, 1), (0, -1)), ((1, 0), (-1, 0)), ((1, 1), (-1, -1)), ((1, -1), (-1, 1)))


def _byte_set(what: str, name: str, members) -> int:
    ms = [members] if isinstance(members, int) and not isinstance(members, bool) else list(members)
    if any(isinstance(c, bool) or int(c) != c or not 0 <= int(c) <= LV_CONTOUR_MAX_BYTE for c in ms) or len({int(c) for c in ms}) != len(ms):
        raise GdkvmError(f"{what}: {name} = {ms} must be distinct integers in 0..{LV_CONTOUR_MAX_BYTE}")
    bits = 0
    for c in ms:
        bits |= 1 << int(c)
    return bits


def _lv_contour_host(m: torch.Tensor, sp: Optional[torch.Tensor], cls: int, wall: int, base: int) -> torch.Tensor:
    """The rule of gdkvm_lv_contour for the frames m [F, H, W] (uint8, CPU) in int64: rec [F, 16].  sp: int32 [F, 2] or None."""
    F, H, W = m.shape
    rec = torch.zeros((F, 16), dtype=torch.int64)
    if F == 0:
        return rec
    pad = torch.nn.functional.pad(m.to(torch.int64), (1, 1, 1, 1), value=0)      # a position outside the frame reads as byte 0
    inside = torch.zeros((H + 2, W + 2), dtype=torch.bool)
    inside[1:-1, 1:-1] = True
    lut = torch.zeros((256, 3), dtype=torch.bool)
    for b in range(LV_CONTOUR_MAX_BYTE + 1):
        lut[b] = torch.tensor([b == cls, bool((wall >> b) & 1), bool((base >> b) & 1)])
    planes = lut[pad]                                                             # [F, H + 2, W + 2, 3]
    C = (planes[..., 0] & inside)[:, 1:-1, 1:-1]
    ys = torch.arange(H, dtype=torch.int64)[None, :, None]
    xs = torch.arange(W, dtype=torch.int64)[None, None, :]
    rec[:, 0] = C.sum((1, 2))
    for s in (0, 1):
        X = planes[..., 1 + s]
        for d, pair in enumerate(_CONTOUR_NEIGHBOURS):
            for dy, dx in pair:
                hit = C & X[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
                rec[:, 1 + 4 * s + d] += hit.sum((1, 2))
                if s == 1 and d < 2:
                    rec[:, 9] += (hit * (2 * xs + dx)).sum((1, 2))
                    rec[:, 10] += (hit * (2 * ys + dy)).sum((1, 2))
    nb = rec[:, 5] + rec[:, 6]
    has = nb > 0
    den = torch.where(has, 2 * nb, torch.ones_like(nb))
    bx2 = torch.div(2 * rec[:, 9] + nb, den, rounding_mode="floor")
    by2 = torch.div(2 * rec[:, 10] + nb, den, rounding_mode="floor")
    ry = torch.ones(F, dtype=torch.int64) if sp is None else sp[:, 0].to(torch.int64)
    rx = torch.ones(F, dtype=torch.int64) if sp is None else sp[:, 1].to(torch.int64)
    d2 = (ry[:, None, None] * (2 * ys - by2[:, None, None])) ** 2 + (rx[:, None, None] * (2 * xs - bx2[:, None, None])) ** 2
    d2 = torch.where(C, d2, torch.full_like(d2, -1)).reshape(F, -1)
    best = d2.amax(1)
    idx = torch.arange(H * W, dtype=torch.int64)[None, :].expand(F, -1)
    apex = torch.where(d2 == best[:, None], idx, torch.full_like(idx, H * W)).amin(1)                # ties: the smallest y W + x
    minus = torch.full_like(nb, -1)
    rec[:, 11], rec[:, 12], rec[:, 13] = torch.where(has, bx2, minus), torch.where(has, by2, minus), torch.where(has, apex, minus)
    rec[:, 14] = torch.where(has, best, torch.zeros_like(best))
    if sp is not None:
        bad = ((sp < 1) | (sp > SPACING_UM_MAX)).any(1)
        rec[bad] = -1
    return rec


def lv_contour(mask: torch.Tensor, cls: int = 1, wall=(2,), base=(3,), spacing_um: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gdkvm_lv_contour: per frame of mask [..., H, W] uint8 the contour record of class `cls` (0..31) against the byte sets `wall` and `base`
    (sequences of distinct bytes in 0..31, disjoint, without cls; wall non-empty, base may be empty): rec int64 [..., 16] = n, N_E N_S N_SE
    N_SW of the wall interface, the same of the base interface, SX2 SY2, the base point bx2 by2 in half pixels, the apex's y W + x, D2 at the
    apex, 0 (definition: include/gdkvm.h; every word an exact integer; without a base interface words 11-13 are -1).  CAMUS: cls = cavity,
    wall = myocardium, base = atrium; a binary mask takes wall = (0,), base = () and has no landmarks.  spacing_um int32 [..., 2] = (row_um,
    col_um), broadcast over the leading dimensions, only moves the apex (D2 in um^2 x 4); None: pixels.  contour_lengths turns the record
    into lengths.  The mask may start at any byte address.  CPU tensors take the same rule in torch, so the wrapper works without a GPU."""
    what = "lv_contour"
    lead, frames, H, W = _mask_frames(what, mask, cls)
    if isinstance(cls, bool) or int(cls) != cls or not 0 <= int(cls) <= LV_CONTOUR_MAX_BYTE:
        raise GdkvmError(f"{what}: cls = {cls} outside 0..{LV_CONTOUR_MAX_BYTE}")
    cls = int(cls)
    wall_set, base_set = _byte_set(what, "wall", wall), _byte_set(what, "base", base)
    if wall_set == 0:
        raise GdkvmError(f"{what}: wall is empty")
    if wall_set & base_set:
        raise GdkvmError(f"{what}: wall and base overlap")
    if (wall_set | base_set) >> cls & 1:
        raise GdkvmError(f"{what}: wall / base holds cls = {cls}")
    if not mask.is_cuda:
        if not mask.is_contiguous():
            raise GdkvmError("GDKVM ops need contiguous tensors")
        sp = None if spacing_um is None else _spacing_frames(what, spacing_um, lead, mask.device).reshape(frames, 2)
        return _lv_contour_host(mask.reshape(frames, H, W), sp, cls, wall_set, base_set).reshape(lead + (16,))
    dev = _dev(mask)
    sp = None if spacing_um is None else _spacing_frames(what, spacing_um, lead, dev)
    rec = torch.empty(lead + (16,), dtype=torch.int64, device=dev)
    _call("gdkvm_lv_contour", dev, mask, sp, rec, frames, H, W, cls, wall_set, base_set)
    return rec


def contour_lengths(rec: torch.Tensor, spacing_um: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The three lengths of lv_contour's records, float64 [..., 3] = L_wall (the endocardial contour), L_base (the annulus width), L_axis
    (apex to base point), on rec's device: the Cauchy-Crofton length over the four lattice directions, weighted by their angular sectors
    (include/gdkvm.h), fp64 with one rounding per operation.  spacing_um int32 [..., 2] as lv_contour took it: mm; None: pixels.  L_axis is
    0 without a base interface; a -1 record (spacing out of range) gives -1."""
    if rec.dtype != torch.int64 or rec.dim() < 1 or rec.shape[-1] != 16:
        raise GdkvmError(f"contour_lengths: rec must be int64 [..., 16], got {rec.dtype} {tuple(rec.shape)}")
    lead = tuple(rec.shape[:-1])
    r = rec.to(torch.float64)
    if spacing_um is None:
        ry = rx = torch.ones(lead, dtype=torch.float64, device=rec.device)
        unit = 1.0
    else:
        sp = _spacing_frames("contour_lengths", spacing_um, lead, rec.device).to(torch.float64)
        ry, rx = sp[..., 0], sp[..., 1]
        unit = 1000.0
    phi = torch.atan2(ry, rx)
    delta = (ry * rx) / torch.sqrt(ry * ry + rx * rx)
    out = []
    for s in (0, 1):
        ne, ns, nd = r[..., 1 + 4 * s], r[..., 2 + 4 * s], r[..., 3 + 4 * s] + r[..., 4 + 4 * s]
        out.append(0.5 * (phi * (ne * ry) + (math.pi / 2 - phi) * (ns * rx) + (math.pi / 4) * (nd * delta)))
    out.append(torch.sqrt(r[..., 14].clamp(min=0.0)) / 2.0)
    res = torch.stack(out, -1) / unit
    return torch.where((rec[..., 0] < 0)[..., None], torch.full_like(res, -1.0), res)


def lv_strain(length: torch.Tensor, npix: torch.Tensor, ed_es: torch.Tensor, min_pixels: int = 1):
    """Longitudinal strain of clips from a length curve, torch fp64 on the inputs' device (a few operations on [B, T]: no kernel).  length
    float64 [B, T] (contour_lengths' L_wall, or L_axis for the long-axis shortening), npix int64 [B, T] (rec[..., 0]), ed_es = lv_ef's
    ed_es_nvalid int32 [B, 3].  Frame t is valid when npix >= min_pixels and length > 0.  The strain curve is e_t = (L_t - L_ED) / L_ED, GLS
    = e_ES; the peak strain is the minimum of e_t over the valid frames, ties to the lowest t.  ok holds when ed >= 0 and both picked frames
    are valid.  Returns (curve float64 [B, T], 0 at invalid frames; gls_peak float64 [B, 3] = GLS, peak strain, L_ED; peak_frame int64 [B];
    ok bool [B]); a clip that is not ok has curve = gls_peak = 0 and peak_frame = -1."""
    if length.dim() != 2 or length.dtype != torch.float64:
        raise GdkvmError(f"lv_strain: length must be float64 [B, T], got {length.dtype} {tuple(length.shape)}")
    B, T = length.shape
    if npix.dtype != torch.int64 or tuple(npix.shape) != (B, T):
        raise GdkvmError(f"lv_strain: npix must be int64 {(B, T)}, got {npix.dtype} {tuple(npix.shape)}")
    if ed_es.dim() != 2 or tuple(ed_es.shape) != (B, 3) or torch.is_floating_point(ed_es):
        raise GdkvmError(f"lv_strain: ed_es must be an integer tensor {(B, 3)}, got {ed_es.dtype} {tuple(ed_es.shape)}")
    if T < 1:
        raise GdkvmError("lv_strain: T = 0")
    valid = (npix >= int(min_pixels)) & (length > 0)
    ed, es = ed_es[:, 0].to(torch.int64), ed_es[:, 1].to(torch.int64)
    picked = (ed >= 0) & (es >= 0) & (ed < T) & (es < T)
    ed_c, es_c = ed.clamp(0, T - 1)[:, None], es.clamp(0, T - 1)[:, None]
    ok = picked & valid.gather(1, ed_c)[:, 0] & valid.gather(1, es_c)[:, 0]
    l_ed = torch.where(ok, length.gather(1, ed_c)[:, 0], torch.ones_like(length[:, 0]))
    use = valid & ok[:, None]
    curve = torch.where(use, (length - l_ed[:, None]) / l_ed[:, None], torch.zeros_like(length))
    gls = curve.gather(1, es_c)[:, 0]
    peak = torch.where(use, curve, torch.full_like(curve, float("inf"))).amin(1)
    t = torch.arange(T, dtype=torch.int64, device=length.device)[None, :].expand(B, -1)
    frame = torch.where(use & (curve == peak[:, None]), t, torch.full_like(t, T)).amin(1)
    zero = torch.zeros_like(gls)
    gls_peak = torch.stack([torch.where(ok, gls, zero), torch.where(ok, peak, zero), torch.where(ok, l_ed, zero)], -1)
    return curve, gls_peak, torch.where(ok, frame, torch.full_like(frame, -1)), ok


def beats_summary(pred_summ: torch.Tensor, pred_info: torch.Tensor, ref_summ: torch.Tensor, ref_info: torch.Tensor,
                  ok: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The running sums of a beat-by-beat comparison of lv_beats' (summ, info) of a prediction and of a reference (float64 [11], on the
    inputs' device; sums of batches and of ranks add): ef_summary's eight sums of the mean beat EF over the clips where both sides have
    n_beats >= 1 and n_below == 0, then the clips compared, the clips whose end-systole counts agree, and the sum of |m_pred - m_ref|.
    ok bool [B] (optional): the clips where it is False are not compared at all (a reference that does not cover the clip)."""
    use = torch.ones_like(pred_info[:, 0], dtype=torch.bool) if ok is None else ok.to(torch.bool)
    both = use & (pred_info[:, 0] >= 1) & (pred_info[:, 2] == 0) & (ref_info[:, 0] >= 1) & (ref_info[:, 2] == 0)
    dm = (pred_info[:, 1] - ref_info[:, 1]).abs() * use
    return torch.cat([ef_summary(pred_summ[:, 0], ref_summ[:, 0], both),
                      torch.stack([use.sum(), ((dm == 0) & use).sum(), dm.sum()]).to(torch.float64)])


def beats_stats(sums) -> dict:
    """{ef_stats' keys over the clips with a beat EF on both sides, clips, systole_count_agreement, systole_count_mae} from beats_summary's
    sums (host numbers; 0 when no clip was compared)."""
    st = ef_stats(sums[:8])
    n, agree, dm = (float(v) for v in sums[8:11])
    st.update(clips=int(n), systole_count_agreement=agree / n if n >= 1 else 0.0, systole_count_mae=dm / n if n >= 1 else 0.0)
    return st


def largest_component(mask: torch.Tensor, cls: int = 1, connectivity: int = 4, fill: int = 0, target: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None):
    """gdkvm_largest_component: per frame of mask [..., H, W] uint8 keep the largest connected component of class `cls` (4- or 8-connected;
    ties: the component with the smallest linear index) and write `fill` over the class's other pixels (definition: include/gdkvm.h; every
    output is an exact integer).  Returns (out uint8 like mask, info int32 [..., 8] = components, n, n_kept, label_kept (-1: no pixel of the
    class), removed_hit_cls, removed_hit_fill, 0, 0); the two hit counts say what the removed pixels were in `target` (same shape; 0 without
    one), which is what counts_after_largest needs.  out=mask filters in place; mask, target and out may start at any byte address."""
    lead, frames, H, W = _mask_frames("largest_component", mask, cls, target=target, out=out)
    if int(connectivity) not in (4, 8):
        raise GdkvmError(f"largest_component: connectivity = {connectivity} is neither 4 nor 8")
    if not 0 <= int(fill) <= 255 or int(fill) == int(cls):
        raise GdkvmError(f"largest_component: fill = {fill} must lie in 0..255 and differ from cls = {cls}")
    dev = _dev(mask, target, out)
    if out is None:
        out = torch.empty_like(mask)
    info = torch.empty(lead + (8,), dtype=torch.int32, device=dev)
    # (allocated per call like every workspace of this module: under graph capture it comes from the graph's own pool and is replayed with it)
    ws = _workspace("gdkvm_largest_component_workspace_bytes", dev, frames, H, W, floor=16)
    _call("gdkvm_largest_component", dev, mask, target, out, info, _Ws(ws), frames, H, W, int(cls), int(connectivity), int(fill))
    return out, info


def counts_after_largest(counts: torch.Tensor, info: torch.Tensor, cls: int, fill: int) -> torch.Tensor:
    """The argmax_dice-style counts [..., ncls, 3] = |A n B|, |A|, |B| of the mask largest_component(mask, cls, fill=fill, target=target)
    wrote, from the counts of the unfiltered mask and that call's info [..., 8]: the removed pixels leave class `cls` (|A| -= n - n_kept,
    |A n B| -= removed_hit_cls) and join class `fill` when it is one of the counted classes (|A| += n - n_kept, |A n B| += removed_hit_fill);
    every other entry is unchanged.  Pure torch on either device, integer-exact."""
    if counts.dim() < 2 or counts.shape[-1] != 3 or info.shape[-1] != 8 or tuple(counts.shape[:-2]) != tuple(info.shape[:-1]):
        raise GdkvmError(f"counts_after_largest: counts [..., ncls, 3] and info [..., 8] must share their leading dimensions, got "
                         f"{tuple(counts.shape)} and {tuple(info.shape)}")
    ncls = counts.shape[-2]
    if not 0 <= int(cls) < ncls:
        raise GdkvmError(f"counts_after_largest: cls = {cls} is none of the {ncls} counted classes")
    if torch.is_floating_point(counts):
        raise GdkvmError("counts_after_largest: counts must be integers")
    inf = info.to(counts.dtype)
    removed = inf[..., 1] - inf[..., 2]
    res = counts.clone()
    res[..., int(cls), 0] -= inf[..., 4]
    res[..., int(cls), 1] -= removed
    if 0 <= int(fill) < ncls:
        res[..., int(fill), 0] += inf[..., 5]
        res[..., int(fill), 1] += removed
    return res


def fill_holes(mask: torch.Tensor, cls: int = 1, connectivity: int = 4, max_area: int = 0, target: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None):
    """gdkvm_fill_holes: per frame of mask [..., H, W] uint8 write `cls` over the holes of class `cls`: the components of its complement
    (`connectivity` 4 or 8 is the COMPLEMENT's; 4 is scipy.ndimage.binary_fill_holes' default) that do not reach the frame's border, those of
    at most `max_area` pixels when max_area > 0 (definition: include/gdkvm.h; every output is an exact integer).  Returns (out uint8 like
    mask, info int32 [..., 8] = holes, holes_filled, n, filled, largest_hole, hit_before, hit_filled, n_target); the last three count against
    `target` (same shape; 0 without one) and are what class_counts_after_fill needs.  out=mask fills in place; mask, target and out may
    start at any byte address."""
    lead, frames, H, W = _mask_frames("fill_holes", mask, cls, target=target, out=out)
    if int(connectivity) not in (4, 8):
        raise GdkvmError(f"fill_holes: connectivity = {connectivity} is neither 4 nor 8")
    if isinstance(max_area, bool) or not isinstance(max_area, int) or not 0 <= max_area < 2 ** 31:
        raise GdkvmError(f"fill_holes: max_area = {max_area} must be an integer >= 0 (0 = holes of any size)")
    dev = _dev(mask, target, out)
    if out is None:
        out = torch.empty_like(mask)
    info = torch.empty(lead + (8,), dtype=torch.int32, device=dev)
    # (allocated per call like every workspace of this module: under graph capture it comes from the graph's own pool and is replayed with it)
    ws = _workspace("gdkvm_fill_holes_workspace_bytes", dev, frames, H, W, floor=16)
    _call("gdkvm_fill_holes", dev, mask, target, out, info, _Ws(ws), frames, H, W, int(cls), int(connectivity), int(max_area))
    return out, info


def class_counts_after_fill(info: torch.Tensor) -> torch.Tensor:
    """The argmax_dice-style counts int64 [..., 3] = |A n B|, |A|, |B| of class `cls` in the mask fill_holes(mask, cls, target=target) wrote,
    from that call's info [..., 8]: hit_before + hit_filled, n + filled, n_target.  Pure torch on either device, integer-exact."""
    if info.dim() < 1 or info.shape[-1] != 8 or torch.is_floating_point(info):
        raise GdkvmError(f"class_counts_after_fill: info must be integers [..., 8] (ops.fill_holes), got {info.dtype} {tuple(info.shape)}")
    inf = info.to(torch.int64)
    return torch.stack([inf[..., 5] + inf[..., 6], inf[..., 2] + inf[..., 3], inf[..., 7]], -1)


TEMPORAL_VOTE_MAX_RADIUS = 7


def temporal_vote(mask: torch.Tensor, num_classes: int, radius: int = 1, target: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None):
    """gdkvm_temporal_vote: smooth the label masks of clips over time.  mask [..., T, H, W] uint8 (the leading dimensions are the clips; a
    3-D mask is one clip): every pixel with a label < num_classes (2..8) takes the class most frames of its window t - radius .. t + radius
    (0..7; truncated at the clip's ends) have there; ties go to the pixel's own label, else to the smallest class; bytes >= num_classes
    neither vote nor change (definition: include/gdkvm.h; every output is an exact integer).  Returns (out uint8 like mask, info int32
    [..., T, 4] = changed, flips_in, flips_out, 0 -- pixels whose label changed, and pixels that differ from the previous frame before and
    after the vote --, counts int32 [..., T, num_classes, 3] = argmax_dice's counts of `out` against `target` (same shape), or None without
    a target).  out must not overlap mask; mask, target and out may start at any byte address."""
    if mask.dim() < 3:
        raise GdkvmError(f"temporal_vote: mask must be uint8 [..., T, H, W], got {mask.dtype} {tuple(mask.shape)}")
    lead, frames, H, W = _mask_frames("temporal_vote", mask, 0, target=target, out=out)
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 2 <= num_classes <= 8:
        raise GdkvmError(f"temporal_vote: num_classes = {num_classes!r} must be an integer in 2..8")
    if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= TEMPORAL_VOTE_MAX_RADIUS:
        raise GdkvmError(f"temporal_vote: radius = {radius!r} must be an integer in 0..{TEMPORAL_VOTE_MAX_RADIUS}")
    T = lead[-1]
    if T < 1:
        raise GdkvmError(f"temporal_vote: T = {T} frames per clip, at least 1")
    dev = _dev(mask, target, out)
    if out is None:
        out = torch.empty_like(mask)
    else:
        lo, hi = mask.data_ptr(), mask.data_ptr() + mask.numel()
        if out.data_ptr() < hi and lo < out.data_ptr() + out.numel():
            raise GdkvmError("temporal_vote: out must not overlap mask (later frames read earlier input)")
    clips = frames // T
    info = torch.empty(lead + (4,), dtype=torch.int32, device=dev)
    counts = torch.empty(lead + (num_classes, 3), dtype=torch.int32, device=dev) if target is not None else None
    # (allocated per call like every workspace of this module; the kernel asks for none today)
    ws = _workspace("gdkvm_temporal_vote_workspace_bytes", dev, clips, T, H, W, num_classes, floor=16)
    _call("gdkvm_temporal_vote", dev, mask, target, out, info, counts, _Ws(ws), clips, T, H, W, num_classes, radius)
    return out, info, counts


def vote_summary(info: torch.Tensor, counts: Optional[torch.Tensor], labelled: torch.Tensor) -> torch.Tensor:
    """The running sums of an evaluation with temporal_vote, int64 [ncls * 3 + 5] on the inputs' device: the voted mask's counts [ncls, 3]
    (flattened) over the frames where `labelled` (bool, broadcastable to info[..., 0]), then over ALL frames pixels changed, frames changed,
    flips_in, flips_out and the number of frames.  counts=None leaves the first part out.  Sums of batches and of ranks add.  Pure torch on
    either device, integer-exact."""
    if info.dim() < 2 or info.shape[-1] != 4 or torch.is_floating_point(info):
        raise GdkvmError(f"vote_summary: info must be integers [..., T, 4] (ops.temporal_vote), got {info.dtype} {tuple(info.shape)}")
    inf = info.to(torch.int64)
    tail = torch.stack([inf[..., 0].sum(), (inf[..., 0] > 0).sum(), inf[..., 1].sum(), inf[..., 2].sum(),
                        torch.tensor(inf[..., 0].numel(), dtype=torch.int64, device=info.device)])
    if counts is None:
        return tail
    if counts.dim() < 2 or counts.shape[-1] != 3 or tuple(counts.shape[:-2]) != tuple(info.shape[:-1]) or torch.is_floating_point(counts):
        raise GdkvmError(f"vote_summary: counts must be integers [..., T, ncls, 3] beside info {tuple(info.shape)}, got {counts.dtype} "
                         f"{tuple(counts.shape)}")
    lab = labelled.to(torch.bool).expand(info.shape[:-1])
    head = (counts.to(torch.int64) * lab[..., None, None]).reshape(-1, counts.shape[-2] * 3).sum(0)
    return torch.cat([head, tail])


# GDKVM_MASK_TO_NATIVE_*: the launch geometry of mask_to_native, for tests that want shapes on both sides of it
MASK_TO_NATIVE_MAX_SIDE = 2048
MASK_TO_NATIVE_RUN, MASK_TO_NATIVE_BAND_PIXELS, MASK_TO_NATIVE_MAX_WG, MASK_TO_NATIVE_CLIPS = 16, 4096, 4096, 64


# The two per-clip tables of a ragged call: the argument's name, the pair's names, the upper bound, the unit behind a value, the noun of
# "N ... for M clips", and what becomes of the values
_SIZE_PAIRS = ("sizes", "(h0, w0)", MASK_TO_NATIVE_MAX_SIDE, "", "sizes", "turned into byte offsets")
_SPACING_PAIRS = ("spacing_um", "(ry, rx)", SPACING_UM_MAX, " um", "spacings", "handed to the kernels by value")


def _native_pairs(what: str, table, rows, clips: Optional[int] = None) -> list:
    """[(h0, w0), ...] (table = _SIZE_PAIRS) or [(ry, rx), ...] (_SPACING_PAIRS) as Python integers from a sequence of pairs or a HOST
    integer tensor [clips, 2]; every value in 1..the table's bound.  A device tensor is refused: the sizes decide where every byte goes and
    the spacings travel by value, so both are validated on the host."""
    arg, pair, hi, unit, noun, use = table
    if isinstance(rows, torch.Tensor):
        if rows.device.type != "cpu":
            raise GdkvmError(f"{what}: {arg} must be host integers (a sequence of {pair} or a CPU tensor [clips, 2]): they are validated and "
                             f"{use} before anything is launched, and a device tensor would have to be copied back first")
        if rows.dim() != 2 or rows.shape[1] != 2 or torch.is_floating_point(rows) or rows.dtype == torch.bool:
            raise GdkvmError(f"{what}: {arg} must be an integer tensor [clips, 2] = {pair}, got {rows.dtype} {tuple(rows.shape)}")
        rows = rows.tolist()
    else:
        try:
            rows = [tuple(r) for r in rows]
        except TypeError:
            raise GdkvmError(f"{what}: {arg} must be a sequence of {pair} or a CPU tensor [clips, 2], got {type(rows).__name__}") from None
    out = []
    for b, r in enumerate(rows):
        if len(r) != 2 or any(isinstance(v, bool) or not isinstance(v, int) for v in r):
            raise GdkvmError(f"{what}: {arg}[{b}] = {r!r} is no pair of integers {pair}")
        if not (1 <= r[0] <= hi and 1 <= r[1] <= hi):
            raise GdkvmError(f"{what}: {arg}[{b}] = {r[0]} x {r[1]}{unit} outside 1..{hi}")
        out.append((r[0], r[1]))
    if clips is not None and len(out) != clips:
        raise GdkvmError(f"{what}: {len(out)} {noun} for {clips} clips")
    return out


def _frames_per_clip(what: str, T, words: str = " frames per clip") -> None:
    if isinstance(T, bool) or not isinstance(T, int) or T < 1:
        raise GdkvmError(f"{what}: T = {T!r}{words} must be an integer >= 1")


def _native_offsets(sizes, T: int):
    """(every clip's first byte, the bytes of all): clip b holds T frames of h0 w0 bytes and follows clip b - 1"""
    offs, total = [], 0
    for h0, w0 in sizes:
        offs.append(total)
        total += T * h0 * w0
    return offs, total


_NO_SPACING = object()          # _native_clips' spacing_um of an entry that takes no spacing table (None is a caller's bad table, and refused)


def _native_clips(what: str, sizes, T: int, spacing_um=_NO_SPACING, clips: Optional[int] = None):
    """The tables of a ragged call, validated: (sz = [(h0, w0), ...], sp = [(ry, rx), ...] or None for an entry without a spacing table,
    every clip's first byte, the bytes of all).  T is an integer >= 1 by now (_frames_per_clip)."""
    sz = _native_pairs(what, _SIZE_PAIRS, sizes, clips)
    sp = None if spacing_um is _NO_SPACING else _native_pairs(what, _SPACING_PAIRS, spacing_um, len(sz))
    return (sz, sp) + _native_offsets(sz, T)


def _host_table(pairs) -> torch.Tensor:
    """The host int32 [clips, 2] table of validated pairs that a native entry reads before it launches"""
    return torch.tensor(pairs, dtype=torch.int32).reshape(len(pairs), 2)


def _flat_u8(what: str, name: str, t, n: int, like: Optional[torch.Tensor] = None, note: str = "", contiguous: bool = True) -> None:
    """t is a ragged native buffer: a flat uint8 tensor of at least n bytes, on the device of `like`, contiguous"""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 1 or t.numel() < n:
        raise GdkvmError(f"{what}: {name} must be a flat uint8 tensor of at least {n} bytes (the clips' T h0 w0 in turn{note}), got "
                         f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    if like is not None and t.device != like.device:
        raise GdkvmError("tensors on different devices")
    if contiguous and not t.is_contiguous():
        raise GdkvmError("GDKVM ops need contiguous tensors")


def _native_axis(n_out: int, n_in: int):
    """The rule's two source indices and weights per native index, int64: (i0, i1, w0, w1) with w0 + w1 = 2 n_out"""
    o = torch.arange(n_out, dtype=torch.int64)
    num, den = (2 * o + 1) * n_in - n_out, 2 * n_out
    i0 = torch.div(num, den, rounding_mode="floor")
    f = num - i0 * den
    return i0.clamp(0, n_in - 1), (i0 + 1).clamp(0, n_in - 1), den - f, f


def _mask_to_native_host(m: torch.Tensor, h0: int, w0: int, ncls: int) -> torch.Tensor:
    """The rule of gdkvm_mask_to_native for the frames m [T, H, W] (uint8, CPU) of one clip, in int64: uint8 [T, h0, w0]"""
    ya, yb, wya, wyb = _native_axis(h0, m.shape[-2])
    xa, xb, wxa, wxb = _native_axis(w0, m.shape[-1])
    votes = torch.zeros((m.shape[0], ncls, h0, w0), dtype=torch.int64)
    for ys, wy in ((ya, wya), (yb, wyb)):
        for xs, wx in ((xa, wxa), (xb, wxb)):
            src = m[:, ys][:, :, xs].to(torch.int64)
            w = wy[:, None] * wx[None, :]
            for c in range(ncls):
                votes[:, c] += w * (src == c)
    # the most votes, the smallest class among equals (votes <= 2^24), 255 where nothing voted
    key = (votes * 8 + (7 - torch.arange(ncls, dtype=torch.int64))[None, :, None, None]).amax(1)
    return torch.where(key >= 8, 7 - key % 8, torch.full_like(key, 255)).to(torch.uint8)


def mask_to_native(mask: torch.Tensor, sizes, num_classes: int, target: Optional[torch.Tensor] = None, want_out: bool = True,
                   out: Optional[torch.Tensor] = None):
    """gdkvm_mask_to_native: take the label masks of clips from the network's grid to every clip's own frame size and count them against the
    native tracing in the same pass.  mask [..., T, H, W] uint8 (the leading dimensions are the clips; a 3-D mask is one clip); sizes the
    clips' native (h0, w0), each in 1..2048: a sequence of pairs of Python integers or a HOST integer tensor [clips, 2] (a device tensor is
    refused).  Every native pixel takes the class with the largest bilinear weight among its four source pixels (half-pixel centres, as
    F.interpolate(align_corners=False) on the one-hot planes; exact integers; ties go to the smallest class, bytes >= num_classes (2..8) do
    not vote, 255 where nothing votes; definition: include/gdkvm.h).  The native masks are RAGGED: flat uint8 tensors in which clip b's T
    frames of h0 w0 bytes follow each other and clip b + 1 follows clip b (pack_native builds one, native_frames views one clip of it).
    Returns (out flat uint8, or None with want_out=False; counts int32 [..., T, num_classes, 3] = argmax_dice's counts of out against
    `target` (flat, 255 = unlabelled), or None without a target; offsets = the host list of every clip's first byte).  `out`: a flat uint8
    tensor to write into.  At least one of out / target.  CPU tensors take the same rule in torch, so the wrapper works without a GPU."""
    what = "mask_to_native"
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or mask.dim() < 3:
        raise GdkvmError(f"{what}: mask must be uint8 [..., T, H, W], got {getattr(mask, 'dtype', type(mask))} {tuple(getattr(mask, 'shape', ()))}")
    lead, frames, H, W = _mask_frames(what, mask, 0)
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 2 <= num_classes <= 8:
        raise GdkvmError(f"{what}: num_classes = {num_classes!r} must be an integer in 2..8")
    T = lead[-1]
    if T < 1:
        raise GdkvmError(f"{what}: T = {T} frames per clip, at least 1")
    clips = frames // T
    sz, _, offsets, total = _native_clips(what, sizes, T, clips=clips)
    if target is None and not want_out:
        raise GdkvmError(f"{what}: neither out (want_out=False) nor a target: nothing to do")
    if out is not None and not want_out:
        raise GdkvmError(f"{what}: an out tensor with want_out=False")
    for name, t in (("target", target), ("out", out)):
        if t is not None:
            _flat_u8(what, name, t, total, mask, contiguous=False)     # (contiguity: behind mask's, below or in _dev)
    if not mask.is_cuda:
        # the same rule in torch on the host (no launch; the wrapper's checks and layout are the GPU path's)
        if not mask.is_contiguous() or any(t is not None and not t.is_contiguous() for t in (target, out)):
            raise GdkvmError("GDKVM ops need contiguous tensors")
        m = mask.reshape(clips, T, H, W)
        res = (torch.empty(total, dtype=torch.uint8) if out is None else out) if want_out else None
        counts = torch.zeros((clips, T, num_classes, 3), dtype=torch.int32) if target is not None else None
        cls = torch.arange(num_classes, dtype=torch.uint8)[None, :, None]
        for b, (h0, w0) in enumerate(sz):
            o = _mask_to_native_host(m[b], h0, w0, num_classes)
            if res is not None:
                res[offsets[b]:offsets[b] + T * h0 * w0] = o.reshape(-1)
            if target is not None:
                eo = o.reshape(T, 1, -1) == cls
                et = target[offsets[b]:offsets[b] + T * h0 * w0].reshape(T, 1, -1) == cls
                counts[b] = torch.stack([(eo & et).sum(-1), eo.sum(-1), et.sum(-1)], -1).to(torch.int32)
        return res, (None if counts is None else counts.reshape(lead + (num_classes, 3))), offsets
    dev = _dev(mask, target, out)
    if want_out:
        if out is None:
            out = torch.empty(total, dtype=torch.uint8, device=dev)
        spans = [(mask.data_ptr(), mask.numel(), "mask")] + ([(target.data_ptr(), total, "target")] if target is not None else [])
        for lo, n, name in spans:
            if out.data_ptr() < lo + n and lo < out.data_ptr() + total:
                raise GdkvmError(f"{what}: out must not overlap {name}")
    counts = torch.empty(lead + (num_classes, 3), dtype=torch.int32, device=dev) if target is not None else None
    if clips == 0:
        return out, counts, offsets
    # (allocated per call like every workspace of this module; the kernel asks for none today)
    ws = _workspace("gdkvm_mask_to_native_workspace_bytes", dev, clips, T, H, W, num_classes, floor=16)
    _call("gdkvm_mask_to_native", dev, mask, _host_table(sz), target, out, counts, total, _Ws(ws), clips, T, H, W, num_classes)
    return out, counts, offsets


def _native_view(what: str, flat, sizes, T, b, bpp: int) -> torch.Tensor:
    """Clip b of a ragged native buffer of bpp bytes per pixel as a view: [T, h0, w0], with bpp > 1 [T, h0, w0, bpp]"""
    sz = _native_pairs(what, _SIZE_PAIRS, sizes)
    _frames_per_clip(what, T, "")
    if isinstance(b, bool) or not isinstance(b, int) or not 0 <= b < len(sz):
        raise GdkvmError(f"{what}: clip {b!r} is none of the {len(sz)} clips")
    offsets, total = _native_offsets(sz, T)
    if not isinstance(flat, torch.Tensor) or flat.dim() != 1 or flat.numel() < bpp * total:
        raise GdkvmError(f"{what}: flat must be a 1-D tensor of at least {bpp * total} elements, got {tuple(getattr(flat, 'shape', ()))}")
    h0, w0 = sz[b]
    return flat[bpp * offsets[b]:bpp * (offsets[b] + T * h0 * w0)].view((T, h0, w0) if bpp == 1 else (T, h0, w0, bpp))


def native_frames(flat: torch.Tensor, sizes, T: int, b: int) -> torch.Tensor:
    """Clip b of a ragged native buffer (mask_to_native's out, pack_native's flat) as a [T, h0, w0] view."""
    return _native_view("native_frames", flat, sizes, T, b, 1)


def pack_native(clips) -> Tuple[torch.Tensor, list]:
    """(flat uint8, sizes) from a list of [T, h0, w0] uint8 tensors with one T, on the tensors' device: the ragged layout mask_to_native
    takes as `target`."""
    clips = list(clips)
    if not clips:
        raise GdkvmError("pack_native: no clips")
    T = clips[0].shape[0] if isinstance(clips[0], torch.Tensor) and clips[0].dim() == 3 else None
    for b, c in enumerate(clips):
        if not isinstance(c, torch.Tensor) or c.dtype != torch.uint8 or c.dim() != 3 or c.shape[0] != T:
            raise GdkvmError(f"pack_native: clip {b} must be uint8 [T, h0, w0] with T = {T}, got {getattr(c, 'dtype', type(c))} "
                             f"{tuple(getattr(c, 'shape', ()))}")
        if c.device != clips[0].device:
            raise GdkvmError("tensors on different devices")
    sizes = _native_pairs("pack_native", _SIZE_PAIRS, [(int(c.shape[1]), int(c.shape[2])) for c in clips])
    return torch.cat([c.reshape(-1) for c in clips]), sizes


# GDKVM_FRAMES_FROM_NATIVE_*: the launch geometry of frames_from_native, for tests that want shapes on both sides of it, and its out_dtype codes
FRAMES_FROM_NATIVE_CHUNK_BYTES, FRAMES_FROM_NATIVE_HS_WORDS, FRAMES_FROM_NATIVE_ACC_WORDS = 16368, 5120, 2048
FRAMES_FROM_NATIVE_PART, FRAMES_FROM_NATIVE_BAND_ROWS, FRAMES_FROM_NATIVE_MAX_WG, FRAMES_FROM_NATIVE_CLIPS = 16, 256, 4096, 64
_FRAMES_DTYPES = {torch.uint8: 0, torch.float32: 1, torch.bfloat16: 2}


def _area_weights(n_grid: int, n_native: int) -> torch.Tensor:
    """The rule's overlap weights of one axis, int64 [n_grid, n_native]: max(0, min((i + 1) n0, (k + 1) n) - max(i n0, k n))"""
    i = torch.arange(n_grid, dtype=torch.int64)[:, None]
    k = torch.arange(n_native, dtype=torch.int64)[None, :]
    return (torch.minimum((i + 1) * n_native, (k + 1) * n_grid) - torch.maximum(i * n_native, k * n_grid)).clamp_(min=0)


def _frames_from_native_host(v: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """The rule of gdkvm_frames_from_native for the frames v [T, h0, w0] (uint8, CPU) of one clip, in int64: the bytes q, uint8 [T, H, W]"""
    h0, w0 = v.shape[-2:]
    n = _area_weights(H, h0) @ v.to(torch.int64) @ _area_weights(W, w0).t()
    return torch.div(2 * n + h0 * w0, 2 * h0 * w0, rounding_mode="floor").to(torch.uint8)


def frames_from_native(flat: torch.Tensor, sizes, T: int, grid=None, channels: int = 3, dtype: torch.dtype = torch.float32,
                       out: Optional[torch.Tensor] = None):
    """gdkvm_frames_from_native: take a ragged batch of native-size uint8 clips to the network's grid by an exact-integer area (box) average
    and cast them to the model's input dtype in the same pass.  flat: a flat uint8 tensor in which clip b's T frames of h0 w0 bytes follow
    each other and clip b + 1 follows clip b (pack_native builds one, native_frames views one clip of it); sizes the clips' native (h0, w0),
    each in 1..2048: a sequence of pairs of Python integers or a HOST integer tensor [clips, 2] (a device tensor is refused); grid = (H, W),
    each in 1..1024, any ratio; channels 1..4, every plane the same value; dtype uint8 (the byte q = the box mean rounded half up), float32
    (float(q) * (1 / 255)) or bfloat16 (that rounded once): torch.mul(q, 1 / 255, out=...) bit for bit (definition: include/gdkvm.h).
    Returns (out [clips, T, channels, H, W], offsets = the host list of every clip's first byte in flat).  `out`: a contiguous tensor of
    that shape and dtype to write into.  CPU tensors take the same rule in torch int64, so the wrapper works without a GPU."""
    what = "frames_from_native"
    if not isinstance(flat, torch.Tensor) or flat.dtype != torch.uint8 or flat.dim() != 1:
        raise GdkvmError(f"{what}: flat must be a flat uint8 tensor (the clips' T h0 w0 bytes in turn), got {getattr(flat, 'dtype', type(flat))} "
                         f"{tuple(getattr(flat, 'shape', ()))}")
    _frames_per_clip(what, T)
    try:
        H, W = grid
    except (TypeError, ValueError):
        raise GdkvmError(f"{what}: grid = {grid!r} must be a pair (H, W)") from None
    if any(isinstance(n, bool) or not isinstance(n, int) for n in (H, W)) or not (1 <= H <= LV_MAX_SIDE and 1 <= W <= LV_MAX_SIDE):
        raise GdkvmError(f"{what}: grid = {grid!r} must be integers (H, W), each in 1..{LV_MAX_SIDE}")
    if isinstance(channels, bool) or not isinstance(channels, int) or not 1 <= channels <= 4:
        raise GdkvmError(f"{what}: channels = {channels!r} must be an integer in 1..4")
    if dtype not in _FRAMES_DTYPES:
        raise GdkvmError(f"{what}: dtype {dtype} is none of uint8, float32, bfloat16")
    sz, _, offsets, total = _native_clips(what, sizes, T)
    clips = len(sz)
    if flat.numel() < total:
        raise GdkvmError(f"{what}: the native frames of these sizes take {total} bytes, flat holds {flat.numel()}")
    shape = (clips, T, channels, H, W)
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != dtype or tuple(out.shape) != shape:
            raise GdkvmError(f"{what}: out must be {dtype} {shape}, got {getattr(out, 'dtype', type(out))} {tuple(getattr(out, 'shape', ()))}")
        if out.device != flat.device:
            raise GdkvmError("tensors on different devices")
    if not flat.is_cuda:
        # the same rule in torch on the host (no launch; the wrapper's checks and layout are the GPU path's)
        if not flat.is_contiguous() or (out is not None and not out.is_contiguous()):
            raise GdkvmError("GDKVM ops need contiguous tensors")
        res = torch.empty(shape, dtype=dtype) if out is None else out
        for b, (h0, w0) in enumerate(sz):
            q = _frames_from_native_host(flat[offsets[b]:offsets[b] + T * h0 * w0].view(T, h0, w0), H, W)[:, None].expand(T, channels, H, W)
            if dtype == torch.uint8:
                res[b] = q
            else:
                torch.mul(q, 1.0 / 255.0, out=res[b])
        return res, offsets
    dev = _dev(flat, out)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=dev)
    if out.data_ptr() % 16:
        raise GdkvmError(f"{what}: out must be 16-byte aligned")
    if out.data_ptr() < flat.data_ptr() + total and flat.data_ptr() < out.data_ptr() + out.numel() * out.element_size():
        raise GdkvmError(f"{what}: out must not overlap flat")
    if clips == 0:
        return out, offsets
    # (allocated per call like every workspace of this module; the kernel asks for none today)
    ws = _workspace("gdkvm_frames_from_native_workspace_bytes", dev, clips, T, channels, H, W, _FRAMES_DTYPES[dtype], floor=16)
    _call("gdkvm_frames_from_native", dev, flat, _host_table(sz), out, total, _Ws(ws), clips, T, channels, H, W, _FRAMES_DTYPES[dtype])
    return out, offsets


# GDKVM_OVERLAY_NATIVE_*: the launch geometry of overlay_native, for tests that want shapes on both sides of it
OVERLAY_NATIVE_RUN, OVERLAY_NATIVE_BAND_RUNS, OVERLAY_NATIVE_BAND_ROWS, OVERLAY_NATIVE_MAX_WG, OVERLAY_NATIVE_CLIPS = 16, 512, 64, 4096, 64
OVERLAY_MAX_WIDTH = 3
# The default colours (R, G, B) of the classes 0..7; class 0 is never drawn.  The prediction's are saturated and far apart, the reference's
# near white, so that a tracing reads as "the light line" whatever class it belongs to.
OVERLAY_PALETTE = ((0, 0, 0), (255, 48, 48), (48, 220, 48), (64, 128, 255), (255, 200, 0), (255, 0, 255), (0, 230, 230), (255, 128, 0))
OVERLAY_REFERENCE_PALETTE = ((0, 0, 0), (255, 255, 255), (255, 255, 190), (200, 255, 255), (255, 215, 255), (225, 225, 225), (215, 255, 215),
                             (255, 235, 215))


def _overlay_palette(what: str, name: str, pal, ncls: int, default) -> torch.Tensor:
    """A palette as a HOST uint8 tensor [ncls, 3]: None is the first ncls colours of `default`; otherwise ncls entries (r, g, b) of integers
    in 0..255, a sequence or a CPU integer tensor.  A device tensor is refused: the colours travel in the kernel arguments."""
    if pal is None:
        pal = default[:ncls]
    if isinstance(pal, torch.Tensor):
        if pal.device.type != "cpu":
            raise GdkvmError(f"{what}: {name} must be host values (a sequence of (r, g, b) or a CPU tensor [num_classes, 3]): the colours are "
                             "validated and handed to the kernel by value")
        if torch.is_floating_point(pal) or pal.dtype == torch.bool:
            raise GdkvmError(f"{what}: {name} must hold integers, got {pal.dtype}")
        pal = pal.tolist()
    try:
        rows = [tuple(r) for r in pal]
    except TypeError:
        raise GdkvmError(f"{what}: {name} must be a sequence of (r, g, b) or a CPU tensor [num_classes, 3], got {type(pal).__name__}") from None
    if len(rows) != ncls:
        raise GdkvmError(f"{what}: {name} has {len(rows)} colours for {ncls} classes")
    for k, r in enumerate(rows):
        if len(r) != 3 or any(isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 255 for v in r):
            raise GdkvmError(f"{what}: {name}[{k}] = {r!r} is no (r, g, b) of integers in 0..255")
    return torch.tensor(rows, dtype=torch.uint8).reshape(ncls, 3)


def _overlay_contour_host(m: torch.Tensor, ncls: int, width: int) -> torch.Tensor:
    """The rule's contour pixels of the frames m [T, h0, w0] (uint8, CPU): bool [T, h0, w0].  The frame is padded with class 0, which differs
    from every class byte, as the outside of the frame does."""
    T, h0, w0 = m.shape
    p = torch.zeros((T, h0 + 2 * width, w0 + 2 * width), dtype=torch.uint8)
    p[:, width:width + h0, width:width + w0] = m
    same = torch.ones(m.shape, dtype=torch.bool)
    for dy in range(-width, width + 1):
        r = width - abs(dy)
        for dx in range(-r, r + 1):
            same &= p[:, width + dy:width + dy + h0, width + dx:width + dx + w0] == m
    return (m >= 1) & (m < ncls) & ~same


def _overlay_native_host(g, m, r, ncls: int, width: int, alpha: int, pal, rpal) -> torch.Tensor:
    """The rule of gdkvm_overlay_native for the frames g, m (and r or None) [T, h0, w0] (uint8, CPU) of one clip, in int64: uint8 [T, h0, w0, 3]"""
    g3 = g.to(torch.int64)[..., None].expand(g.shape + (3,))
    cls = (m >= 1) & (m < ncls)
    k = torch.where(cls, m, torch.zeros_like(m)).to(torch.int64)
    colour = pal.to(torch.int64)[k]
    out = torch.where(cls[..., None], (g3 * (256 - alpha) + colour * alpha + 128) >> 8, g3)
    if r is not None:
        on_r = _overlay_contour_host(r, ncls, width)
        kr = torch.where(on_r, r, torch.zeros_like(r)).to(torch.int64)
        out = torch.where(on_r[..., None], rpal.to(torch.int64)[kr], out)
    out = torch.where(_overlay_contour_host(m, ncls, width)[..., None], colour, out)
    return out.to(torch.uint8)


def overlay_native(grey: torch.Tensor, mask: torch.Tensor, sizes, T: int, num_classes: int, reference: Optional[torch.Tensor] = None,
                   width: int = 2, alpha: int = 96, palette=None, reference_palette=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gdkvm_overlay_native: the picture of a segmentation at every clip's own frame size -- the grey frame, the mask's classes tinted
    (alpha / 256 of the class colour; 0 draws contours only, 256 paints the class solid), the mask's contour opaque in the class colour and,
    with `reference`, that mask's contour in the reference colours where the mask's own contour does not cover it.  A contour pixel of a
    mask holds a class byte k (1 <= k < num_classes, 2..8) and has a pixel within the 4-neighbour distance `width` (1..3) that holds another
    byte or lies outside the frame (definition: include/gdkvm.h).  grey, mask and reference are RAGGED flat uint8 tensors, clip b's T frames
    of h0 w0 bytes in turn (pack_native builds one, mask_to_native returns one, native_frames views one clip); sizes the clips' native
    (h0, w0), each in 1..2048, HOST integers (a device tensor is refused), and so are the palettes: num_classes entries (r, g, b), None for
    OVERLAY_PALETTE / OVERLAY_REFERENCE_PALETTE.  Returns the flat uint8 RGB buffer, three bytes per pixel in the same order
    (native_rgb_frames views one clip of it as [T, h0, w0, 3]); `out`: a flat uint8 tensor of at least three times the pixels to write
    into, overlapping no input.  CPU tensors take the same rule in torch integers, so the wrapper works without a GPU."""
    what = "overlay_native"
    _frames_per_clip(what, T)
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 2 <= num_classes <= 8:
        raise GdkvmError(f"{what}: num_classes = {num_classes!r} must be an integer in 2..8")
    if isinstance(width, bool) or not isinstance(width, int) or not 1 <= width <= OVERLAY_MAX_WIDTH:
        raise GdkvmError(f"{what}: width = {width!r} must be an integer in 1..{OVERLAY_MAX_WIDTH}")
    if isinstance(alpha, bool) or not isinstance(alpha, int) or not 0 <= alpha <= 256:
        raise GdkvmError(f"{what}: alpha = {alpha!r} must be an integer in 0..256")
    sz, _, offsets, total = _native_clips(what, sizes, T)
    clips = len(sz)
    pal = _overlay_palette(what, "palette", palette, num_classes, OVERLAY_PALETTE)
    rpal = _overlay_palette(what, "reference_palette", reference_palette, num_classes, OVERLAY_REFERENCE_PALETTE)
    if not isinstance(grey, torch.Tensor):
        raise GdkvmError(f"{what}: grey must be a flat uint8 tensor, got {type(grey).__name__}")
    _flat_u8(what, "grey", grey, total)
    _flat_u8(what, "mask", mask, total, grey)
    if reference is not None:
        _flat_u8(what, "reference", reference, total, grey)
    if out is not None:
        _flat_u8(what, "out", out, 3 * total, grey, note=", three bytes per pixel")
    else:
        out = torch.empty(3 * total, dtype=torch.uint8, device=grey.device)
    for name, t in (("grey", grey), ("mask", mask), ("reference", reference)):
        if t is not None and total and out.data_ptr() < t.data_ptr() + total and t.data_ptr() < out.data_ptr() + 3 * total:
            raise GdkvmError(f"{what}: out must not overlap {name}")
    if clips == 0:
        return out
    if not grey.is_cuda:
        # the same rule in torch on the host (no launch; the wrapper's checks and layout are the GPU path's)
        for b, (h0, w0) in enumerate(sz):
            lo, hi = offsets[b], offsets[b] + T * h0 * w0
            r = None if reference is None else reference[lo:hi].view(T, h0, w0)
            o = _overlay_native_host(grey[lo:hi].view(T, h0, w0), mask[lo:hi].view(T, h0, w0), r, num_classes, width, alpha, pal, rpal)
            out[3 * lo:3 * hi] = o.reshape(-1)
        return out
    dev = _dev(grey, mask, reference, out)
    # (allocated per call like every workspace of this module; the kernel asks for none today)
    ws = _workspace("gdkvm_overlay_native_workspace_bytes", dev, clips, T, num_classes, width, floor=16)
    _call("gdkvm_overlay_native", dev, grey, mask, reference, _host_table(sz), pal, rpal if reference is not None else None, out, total, _Ws(ws),
          clips, T, num_classes, width, alpha)
    return out


def native_rgb_frames(flat: torch.Tensor, sizes, T: int, b: int) -> torch.Tensor:
    """Clip b of a ragged native RGB buffer (overlay_native's result) as a [T, h0, w0, 3] view: native_frames with three bytes per pixel."""
    return _native_view("native_rgb_frames", flat, sizes, T, b, 3)


def surface_distance(mask: torch.Tensor, target: torch.Tensor, cls: int = 1) -> torch.Tensor:
    """gdkvm_surface_distance: per frame of mask and target [..., H, W] uint8 the surfaces of class `cls` (its pixels with a 4-neighbour
    outside the class or the frame) and the exact squared Euclidean distances from each surface to the other (definition: include/gdkvm.h;
    every output is an exact integer).  Returns surf int64 [..., 8] = nA, nB, hAB, hBA, sAB, sBA, q_lo, q_hi: the surface sizes of mask and
    target, the largest squared distance per direction, the per-direction sums of the distances in units of 2^-16 pixel (each rounded down)
    and the two squared distances that enclose the pooled 95th percentile; an empty surface leaves the six other fields 0.  surface_metrics
    turns it into HD, HD95 and ASSD.  mask and target may start at any byte address."""
    return _surface_distance("gdkvm_surface_distance", mask, target, None, cls)


def surface_metrics(surf: torch.Tensor):
    """(metrics float64 [..., 3] = HD, HD95, ASSD in pixels, valid bool [...]) from surface_distance's surf [..., 8]; valid = both surfaces
    have pixels, and the metrics of an invalid frame are 0.  HD = sqrt(max(hAB, hBA)); HD95 = a + (b - a) (95 (n - 1) mod 100) / 100 with
    a = sqrt(q_lo), b = sqrt(q_hi), n = nA + nB -- the linearly interpolated 95th percentile of the pooled distances (sorting d^2 sorts d);
    ASSD = (sAB / nA + sBA / nB) / 2 / 65536 (at most 2^-16 pixel below the mean of the unrounded distances).  Pure torch on either device."""
    return _surface_metrics("surface_metrics", surf, 1.0, 65536.0)


def surface_distance_mm(mask: torch.Tensor, target: torch.Tensor, spacing_um: torch.Tensor, cls: int = 1) -> torch.Tensor:
    """gdkvm_surface_distance_mm: surface_distance with a pixel spacing -- spacing_um int32 [..., 2] = (row_um, col_um) micrometres per pixel,
    broadcast over mask's leading dimensions.  Returns surf int64 [..., 8] = nA, nB, hAB, hBA (um^2), sAB, sBA (sums of the distances in
    units of 2^-8 um, each rounded down), q_lo, q_hi (um^2); a frame whose spacing (a device tensor's: a host tensor is refused) is outside
    1..4095 holds eight -1.  surface_metrics_mm turns it into HD, HD95 and ASSD in mm."""
    return _surface_distance("gdkvm_surface_distance_mm", mask, target, spacing_um, cls)


def _surface_distance(entry: str, mask, target, spacing_um, cls):
    """surface_distance (spacing_um None) and surface_distance_mm behind their entry point and its workspace query: the spacing in front of surf"""
    what = entry[len("gdkvm_"):]
    lead, frames, H, W = _mask_frames(what, mask, cls, target=target)
    dev = _dev(mask, target)
    sp = () if spacing_um is None else (_spacing_frames(what, spacing_um, lead, dev),)
    surf = torch.empty(lead + (8,), dtype=torch.int64, device=dev)
    ws = _workspace(entry + "_workspace_bytes", dev, frames, H, W, floor=16)
    _call(entry, dev, mask, target, *sp, surf, _Ws(ws), frames, H, W, int(cls))
    return surf


# GDKVM_SURFACE_NATIVE_*: the launch geometry of surface_distance_native, for tests that want shapes on both sides of it
SURFACE_NATIVE_BAND_ROWS, SURFACE_NATIVE_STRIP, SURFACE_NATIVE_MAX_WG, SURFACE_NATIVE_CLIPS = 32, 64, 4096, 64


def _surface_bool(x: torch.Tensor) -> torch.Tensor:
    """The surface of the boolean set x [h, w]: its pixels with a 4-neighbour outside the set or the frame"""
    p = torch.nn.functional.pad(x, (1, 1, 1, 1))
    return x & ~(p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:])


def _directed_d2_host(pa: torch.Tensor, pb: torch.Tensor, ry: int, rx: int) -> torch.Tensor:
    """int64 [len(pa)]: min over q in pb of (ry dy)^2 + (rx dx)^2, brute force over coordinates [n, 2] = (y, x), in chunks of pa"""
    out = torch.empty(pa.shape[0], dtype=torch.int64)
    step = max(1, (1 << 22) // max(1, pb.shape[0]))
    for i in range(0, pa.shape[0], step):
        d = pa[i:i + step, None, :] - pb[None, :, :]
        out[i:i + step] = ((d[..., 0] * ry) ** 2 + (d[..., 1] * rx) ** 2).amin(1)
    return out


def _surface_native_host(m: torch.Tensor, t: torch.Tensor, ry: int, rx: int, cls: int) -> list:
    """The record of gdkvm_surface_distance_native for one frame [h0, w0] (uint8, CPU) as 8 Python ints"""
    pa, pb = _surface_bool(m == cls).nonzero(), _surface_bool(t == cls).nonzero()
    nA, nB = pa.shape[0], pb.shape[0]
    if nA == 0 or nB == 0:
        return [nA, nB, 0, 0, 0, 0, 0, 0]
    dab, dba = _directed_d2_host(pa, pb, ry, rx), _directed_d2_host(pb, pa, ry, rx)
    fixed = lambda d: sum(math.isqrt(int(v) << 16) * int(c) for v, c in zip(*(u.tolist() for u in torch.unique(d, return_counts=True))))
    pooled = torch.sort(torch.cat([dab, dba])).values
    n = nA + nB
    lo = (95 * (n - 1)) // 100
    return [nA, nB, int(dab.max()), int(dba.max()), fixed(dab), fixed(dba), int(pooled[lo]), int(pooled[min(lo + 1, n - 1)])]


def surface_distance_native(mask: torch.Tensor, target: torch.Tensor, sizes, T: int, spacing_um, cls: int = 1) -> torch.Tensor:
    """gdkvm_surface_distance_native: surface_distance_mm at every clip's own frame size.  mask and target are RAGGED flat uint8 tensors,
    clip b's T frames of h0 w0 bytes in turn (mask_to_native returns one, pack_native builds one); sizes the clips' native (h0, w0), each in
    1..2048, and spacing_um the micrometres per NATIVE pixel (ry, rx) of every clip, each in 1..4095: both HOST integers, a sequence of
    pairs or a CPU integer tensor [clips, 2] (a device tensor is refused).  Returns surf int64 [clips, T, 8] = nA, nB, hAB, hBA (um^2),
    sAB, sBA (sums of the distances in units of 2^-8 um, each rounded down), q_lo, q_hi (um^2), surface_distance_mm's record (definition:
    include/gdkvm.h): surface_metrics_mm, surface_summary and surface_stats apply unchanged.  mask and target may start at any byte
    address.  CPU tensors take the same rule in torch (brute force over the surface pixels' coordinates in int64), so the wrapper works
    without a GPU."""
    what = "surface_distance_native"
    _frames_per_clip(what, T)
    if isinstance(cls, bool) or not isinstance(cls, int) or not 0 <= cls <= 254:
        raise GdkvmError(f"{what}: cls = {cls!r} must be an integer in 0..254")
    sz, sp, offsets, total = _native_clips(what, sizes, T, spacing_um)
    clips = len(sz)
    if not isinstance(mask, torch.Tensor):
        raise GdkvmError(f"{what}: mask must be a flat uint8 tensor, got {type(mask).__name__}")
    _flat_u8(what, "mask", mask, total)
    _flat_u8(what, "target", target, total, mask)
    if not mask.is_cuda:
        # the same rule in torch on the host (no launch; the wrapper's checks and layout are the GPU path's)
        surf = torch.zeros((clips, T, 8), dtype=torch.int64)
        for b, (h0, w0) in enumerate(sz):
            m = mask[offsets[b]:offsets[b] + T * h0 * w0].view(T, h0, w0)
            t = target[offsets[b]:offsets[b] + T * h0 * w0].view(T, h0, w0)
            for f in range(T):
                surf[b, f] = torch.tensor(_surface_native_host(m[f], t[f], sp[b][0], sp[b][1], cls), dtype=torch.int64)
        return surf
    dev = _dev(mask, target)
    surf = torch.empty((clips, T, 8), dtype=torch.int64, device=dev)
    if clips == 0:
        return surf
    ws = _workspace("gdkvm_surface_distance_native_workspace_bytes", dev, clips, T, total, T * sum(h0 for h0, _ in sz), floor=16)
    _call("gdkvm_surface_distance_native", dev, mask, target, _host_table(sz), _host_table(sp), surf, total, _Ws(ws), clips, T, cls)
    return surf


# GDKVM_LV_NATIVE_*: the launch geometry of lv_measure_native, for tests that want shapes on both sides of it
LV_NATIVE_BAND_ROWS, LV_NATIVE_MAX_WG, LV_NATIVE_CLIPS = 32, 4096, 64
_LV_Q = 1 << 16
_I64_MAX, _I64_MIN = (1 << 63) - 1, -(1 << 63)


def _lv_native_axis(n: int, sx: int, sy: int, sxx: int, sxy: int, syy: int, ry: int, rx: int):
    """Steps 2 and 3' of gdkvm_lv_measure_mm in Python integers and floats (IEEE fp64, one rounding per operation, sqrt and division correctly
    rounded; round() is half to even, as rint): (Vx, Vy, E, k)"""
    g = math.gcd(ry, rx)
    py, px = ry // g, rx // g
    pm = max(px, py)
    A, B, C = n * sxx - sx * sx, n * sxy - sx * sy, n * syy - sy * sy
    a = float(px * px) * float(A) - float(py * py) * float(C)
    b = 2.0 * (float(px * py) * float(B))
    r = math.sqrt(a * a + b * b)
    if r == 0.0:
        vx, vy = 0.0, 1.0
    elif a >= 0.0:
        vx, vy = a + r, b
    else:
        vx, vy = b, r - a
    nrm = math.sqrt(vx * vx + vy * vy)
    ux, uy = vx / nrm, vy / nrm
    if uy < 0.0 or (uy == 0.0 and ux < 0.0):
        ux, uy = -ux, -uy
    ex, ey = ux * float(px), uy * float(py)
    e = math.sqrt(ex * ex + ey * ey)
    return (int(round((ux * float(px * _LV_Q)) / float(pm))), int(round((uy * float(py * _LV_Q)) / float(pm))),
            int(round((e * float(_LV_Q)) / float(pm))), e * float(g))


def _lv_native_host(m: torch.Tensor, ry: int, rx: int, cls: int, D: int):
    """The records of gdkvm_lv_measure_native for one frame [h0, w0] (uint8, CPU): (stats 12 ints, disks D ints, geom 6 floats, band rows
    [ceil(h0 / LV_NATIVE_BAND_ROWS)][8 + D] ints).  int64 tensors for what the header bounds below 2^63, Python integers for A, B and C."""
    nbands = (m.shape[0] + LV_NATIVE_BAND_ROWS - 1) // LV_NATIVE_BAND_ROWS
    ys, xs = (m == cls).nonzero(as_tuple=True)
    n = int(xs.numel())
    if n == 0:
        return [0] * 12, [0] * D, [0.0] * 6, [[0] * (8 + D) for _ in range(nbands)]
    band = torch.div(ys, LV_NATIVE_BAND_ROWS, rounding_mode="floor")
    per_band = lambda v: torch.zeros(nbands, dtype=torch.int64).index_add_(0, band, v)
    mom = [per_band(v) for v in (torch.ones_like(xs), xs, ys, xs * xs, xs * ys, ys * ys)]
    tot = [int(v.sum()) for v in mom]
    sx, sy = tot[1], tot[2]
    Vx, Vy, E, k = _lv_native_axis(*tot, ry, rx)
    t = (n * xs - sx) * Vx + (n * ys - sy) * Vy               # |.| < 2^50
    b_min = torch.full((nbands,), _I64_MAX, dtype=torch.int64).scatter_reduce_(0, band, t, "amin")
    b_max = torch.full((nbands,), _I64_MIN, dtype=torch.int64).scatter_reduce_(0, band, t, "amax")
    tmin, tmax = int(t.min()), int(t.max())
    P1 = n * E
    Lt = tmax - tmin + P1
    lo = D * (t - tmin)
    hi = lo + D * P1
    w_band = [per_band((torch.clamp(hi, max=(j + 1) * Lt) - torch.clamp(lo, min=j * Lt)).clamp_(min=0)) for j in range(D)]
    disks = [int(w.sum()) for w in w_band]
    L = ((float(Lt) / float(P1)) * k) / 1000.0
    pix = float(ry * rx) / 1e6
    s = 0.0
    for w in disks:
        aj = (float(w) / float(D * P1)) * pix
        s = s + aj * aj
    geom = [L, ((math.pi * D) * s) / (4.0 * L) / 1000.0, ((float(sx) / float(n)) * float(rx)) / 1000.0,
            ((float(sy) / float(n)) * float(ry)) / 1000.0, k, float(n * ry * rx) / 1e6]
    rows = torch.stack(mom + [b_min, b_max] + w_band, 1).tolist()
    return tot + [Vx, Vy, tmin, tmax, Lt, E], disks, geom, rows


def lv_measure_native(mask: torch.Tensor, sizes, T: int, spacing_um, cls: int = 1, disks: int = 20, want_bands: bool = False):
    """gdkvm_lv_measure_native: lv_measure_mm at every clip's own frame size.  mask is a RAGGED flat uint8 tensor, clip b's T frames of
    h0 w0 bytes in turn (mask_to_native returns one, pack_native builds one); sizes the clips' native (h0, w0), each in 1..2048, and
    spacing_um the micrometres per NATIVE pixel (ry, rx) of every clip, each in 1..4095: both HOST integers, a sequence of pairs or a CPU
    integer tensor [clips, 2] (a device tensor is refused).  Returns (stats int64 [clips, T, 12] = n sx sy sxx sxy syy Vx Vy tmin tmax Lt E,
    disks int64 [clips, T, D], geom float64 [clips, T, 6] = L in mm, V in mL, cx, cy in mm, k, area in mm^2), lv_measure_mm's records
    (definition: include/gdkvm.h): lv_ef, lv_beats and lv_biplane (with native_spacing_frames) apply unchanged.  want_bands: also the
    per-band partials, int64 [bands, 8 + D] in clip, frame, band order with ceil(h0 / LV_NATIVE_BAND_ROWS) bands per frame = n sx sy sxx
    sxy syy tmin tmax W_0 .. W_(D-1) of the band's rows.  mask may start at any byte address.  CPU tensors take the same rule in torch
    and Python integers, so the wrapper works without a GPU."""
    what = "lv_measure_native"
    _frames_per_clip(what, T)
    if isinstance(cls, bool) or not isinstance(cls, int) or not 0 <= cls <= 254:
        raise GdkvmError(f"{what}: cls = {cls!r} must be an integer in 0..254")
    if isinstance(disks, bool) or not isinstance(disks, int) or not 1 <= disks <= LV_MAX_DISKS:
        raise GdkvmError(f"{what}: disks = {disks!r} must be an integer in 1..{LV_MAX_DISKS}")
    sz, sp, offsets, total = _native_clips(what, sizes, T, spacing_um)
    clips = len(sz)
    _flat_u8(what, "mask", mask, total)
    nbands = T * sum((h0 + LV_NATIVE_BAND_ROWS - 1) // LV_NATIVE_BAND_ROWS for h0, _ in sz)
    if not mask.is_cuda:
        # the same rule in torch on the host (no launch; the wrapper's checks and layout are the GPU path's)
        stats = torch.zeros((clips, T, 12), dtype=torch.int64)
        dk = torch.zeros((clips, T, disks), dtype=torch.int64)
        geom = torch.zeros((clips, T, 6), dtype=torch.float64)
        rows = []
        for b, (h0, w0) in enumerate(sz):
            m = mask[offsets[b]:offsets[b] + T * h0 * w0].view(T, h0, w0)
            for f in range(T):
                s, d, g, r = _lv_native_host(m[f], sp[b][0], sp[b][1], cls, disks)
                stats[b, f], dk[b, f] = torch.tensor(s, dtype=torch.int64), torch.tensor(d, dtype=torch.int64)
                geom[b, f] = torch.tensor(g, dtype=torch.float64)
                rows += r
        bands = torch.tensor(rows, dtype=torch.int64).reshape(nbands, 8 + disks)
        return (stats, dk, geom, bands) if want_bands else (stats, dk, geom)
    dev = _dev(mask)
    stats = torch.empty((clips, T, 12), dtype=torch.int64, device=dev)
    dk = torch.empty((clips, T, disks), dtype=torch.int64, device=dev)
    geom = torch.empty((clips, T, 6), dtype=torch.float64, device=dev)
    bands = torch.empty((nbands, 8 + disks), dtype=torch.int64, device=dev)
    if clips:
        _call("gdkvm_lv_measure_native", dev, mask, _host_table(sz), _host_table(sp), stats, dk, geom, bands, total, nbands, clips, T, cls, disks)
    return (stats, dk, geom, bands) if want_bands else (stats, dk, geom)


def native_spacing_frames(spacing_um, T: int, device) -> torch.Tensor:
    """int32 [clips, T, 2] on `device`: every clip's native (ry, rx) for each of its T frames, the table lv_biplane reads beside the
    records of lv_measure_native.  spacing_um as there: HOST integers, validated here before anything is copied."""
    what = "native_spacing_frames"
    _frames_per_clip(what, T)
    if not isinstance(spacing_um, torch.Tensor):
        spacing_um = list(spacing_um) if hasattr(spacing_um, "__iter__") else spacing_um
    sp = _native_pairs(what, _SPACING_PAIRS, spacing_um, len(spacing_um) if hasattr(spacing_um, "__len__") else 0)
    return torch.tensor(sp, dtype=torch.int32).reshape(len(sp), 1, 2).expand(len(sp), T, 2).contiguous().to(device)


def surface_metrics_mm(surf: torch.Tensor):
    """(metrics float64 [..., 3] = HD, HD95, ASSD in mm, valid bool [...]) from surface_distance_mm's surf [..., 8]: surface_metrics'
    formulas with sqrt(.) / 1000 for the squared distances (um^2) and / 256 / 1000 for the sums (2^-8 um).  A record of -1 (a spacing out
    of range) is invalid, like one with an empty surface; the metrics of an invalid frame are 0."""
    return _surface_metrics("surface_metrics_mm", surf, 1000.0, 256.0)


def _surface_metrics(what: str, surf, unit: float, sum_scale: float):
    """surface_metrics (unit 1: pixels, sums in 2^-16) and surface_metrics_mm (unit 1000: um -> mm, sums in 2^-8; negative fields, the -1
    record, count as 0): one formula, distances / unit and sums / sum_scale / unit (a division by 1.0 changes no bit)"""
    if surf.shape[-1] != 8 or torch.is_floating_point(surf):
        raise GdkvmError(f"{what}: surf must be integers [..., 8], got {surf.dtype} {tuple(surf.shape)}")
    s = surf.to(torch.int64)
    nA, nB = s[..., 0], s[..., 1]
    valid = (nA > 0) & (nB > 0)
    d = (s if unit == 1.0 else s.clamp(min=0)).to(torch.float64)
    hd = torch.maximum(d[..., 2], d[..., 3]).sqrt() / unit
    a, b = d[..., 6].sqrt() / unit, d[..., 7].sqrt() / unit
    frac = ((95 * (nA + nB - 1).clamp(min=0)) % 100).to(torch.float64) / 100.0
    hd95 = a + (b - a) * frac
    assd = (d[..., 4] / d[..., 0].clamp(min=1.0) + d[..., 5] / d[..., 1].clamp(min=1.0)) / 2.0 / sum_scale / unit
    metrics = torch.stack([hd, hd95, assd], -1) * valid.unsqueeze(-1).to(torch.float64)
    return metrics, valid


def surface_summary(metrics: torch.Tensor, valid: torch.Tensor, surf: torch.Tensor, labelled: torch.Tensor) -> torch.Tensor:
    """The five running sums of a surface-distance evaluation over the frames where `labelled` (bool, the shape of `valid`): frames counted
    (labelled and valid), frames where exactly one of the two surfaces is empty (no distance exists; they are reported, not averaged),
    sum HD, sum HD95, sum ASSD (float64 [5], on the inputs' device).  Sums of batches and of ranks add; surface_stats makes the means."""
    lab = labelled.to(torch.bool).expand(valid.shape)
    k = (valid & lab).to(torch.float64)
    one = (((surf[..., 0] > 0) != (surf[..., 1] > 0)) & lab).to(torch.float64)
    m = metrics.to(torch.float64) * k.unsqueeze(-1)
    return torch.stack([k.sum(), one.sum(), m[..., 0].sum(), m[..., 1].sum(), m[..., 2].sum()])


def surface_stats(sums) -> dict:
    """{frames, frames_one_empty, hd_mean, hd95_mean, assd_mean} from surface_summary's sums (host numbers, pixels; 0 when no frame counts)."""
    n, one, hd, hd95, assd = (float(v) for v in sums)
    d = n if n >= 1 else 1.0
    return {"frames": int(n), "frames_one_empty": int(one), "hd_mean": hd / d, "hd95_mean": hd95 / d, "assd_mean": assd / d}


ADAMW_SCHEDULES = {"constant": 0, "cosine": 1, "poly": 2}      # GDKVM_SCHEDULE_*
ADAMW_STATE_WORDS = 8                                          # GDKVM_ADAMW_STATE_BYTES / 8


def adamw_state(device) -> torch.Tensor:
    """The persistent state block of adamw_step, zeroed: int64 [8] -- [0] step, [1] skipped, [2:5] viewed as float64 the last gradient norm,
    clip coefficient and learning rate, the rest private to the kernels."""
    return torch.zeros(ADAMW_STATE_WORDS, dtype=torch.int64, device=device)


def adamw_workspace(device, tensors: int, total_elems: int) -> torch.Tensor:
    """A workspace for adamw_step over `tensors` tensors of `total_elems` elements in all (one fp32 partial per 4096-element chunk)."""
    return _workspace("gdkvm_adamw_workspace_bytes", device, int(tensors), int(total_elems), floor=16)


def adamw_step(addresses: torch.Tensor, counts: torch.Tensor, decays: torch.Tensor, state: torch.Tensor, workspace: torch.Tensor, *,
               lr: float, betas=(0.9, 0.999), eps: float = 1e-8, max_norm: float = 0.0, ema_decay: float = 0.0, schedule: str = "constant",
               warmup_steps: int = 0, total_steps: int = 0, min_lr_ratio: float = 0.0, poly_power: float = 0.9) -> None:
    """gdkvm_adamw_step (definition: include/gdkvm.h): one AdamW step with global-norm clipping, the scheduled learning rate, the non-finite
    guard and the EMA over the tensors whose DEVICE addresses the HOST tensor `addresses` holds -- int64 [5, n] on the CPU, rows: parameter,
    gradient, exp_avg, exp_avg_sq, EMA copy (0 = none; the row is ignored while ema_decay == 0) -- with `counts` int64 [n] and `decays` fp32 [n]
    on the CPU too.  All tensors addressed are fp32 on state's device, and gradient / moments / EMA pair with the parameter by address.  `state`
    (adamw_state) and `workspace` (adamw_workspace) live on the device; three kernels on the current stream, nothing synchronises."""
    n = int(counts.numel())
    if (addresses.device.type != "cpu" or addresses.dtype != torch.int64 or tuple(addresses.shape) != (5, n) or not addresses.is_contiguous()
            or counts.device.type != "cpu" or counts.dtype != torch.int64 or not counts.is_contiguous()
            or decays.device.type != "cpu" or decays.dtype != torch.float32 or tuple(decays.shape) != (n,) or not decays.is_contiguous()):
        raise GdkvmError("adamw_step: addresses int64 [5, n], counts int64 [n] and decays fp32 [n] must be contiguous CPU tensors")
    if schedule not in ADAMW_SCHEDULES:
        raise GdkvmError(f"adamw_step: schedule = {schedule!r}, one of {sorted(ADAMW_SCHEDULES)}")
    dev = _dev(state, workspace)
    if state.dtype != torch.int64 or state.numel() != ADAMW_STATE_WORDS:
        raise GdkvmError(f"adamw_step: state must be int64 [{ADAMW_STATE_WORDS}] (ops.adamw_state)")
    if n == 0:
        return
    a = addresses
    _call("gdkvm_adamw_step", dev, a[0], a[1], a[2], a[3], a[4] if ema_decay > 0 else None, counts, decays, n, state, _Ws(workspace),
          float(lr), float(betas[0]), float(betas[1]), float(eps), float(max_norm), float(ema_decay), float(min_lr_ratio), float(poly_power),
          int(warmup_steps), int(total_steps), ADAMW_SCHEDULES[schedule])
