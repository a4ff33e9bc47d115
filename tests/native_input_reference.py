"""The rule of gdkvm_frames_from_native (include/gdkvm.h) restated in numpy int64 from the weight formula: dense weight matrices Wy @ v @ Wx.T,
independent of gdkvm_amd.ops' host path, and the three output dtypes.  The yardstick of tests/test_native_input_cpu.py and
tests/test_native_input_gpu.py; computed once per shape and handed out read-only."""
import numpy as np


def weights(n_grid, n_native):
    """w(i, k) = max(0, min((i + 1) n0, (k + 1) n) - max(i n0, k n)), int64 [n_grid, n_native]"""
    i = np.arange(n_grid, dtype=np.int64)[:, None]
    k = np.arange(n_native, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((i + 1) * n_native, (k + 1) * n_grid) - np.maximum(i * n_native, k * n_grid))


def numerators(v, H, W):
    """N [..., H, W] int64 of the native frames v [..., h0, w0] uint8"""
    v = np.asarray(v)
    assert v.dtype == np.uint8 and v.ndim >= 2
    return weights(H, v.shape[-2]) @ v.astype(np.int64) @ weights(W, v.shape[-1]).T


def area_bytes(v, H, W):
    """q [..., H, W] uint8 = floor((2 N + h0 w0) / (2 h0 w0))"""
    v = np.asarray(v)
    a = v.shape[-2] * v.shape[-1]
    n = numerators(v, H, W)
    assert n.max(initial=0) <= 255 * a and 2 * n.max(initial=0) + a < 2 ** 32
    return ((2 * n + a) // (2 * a)).astype(np.uint8)


def to_float32(q):
    """float(q) * (1.0f / 255.0f): one fp32 product"""
    return q.astype(np.float32) * np.float32(1.0 / 255.0)


def to_bf16_bits(q):
    """that fp32 value rounded once to bfloat16, to nearest even: the uint16 bit patterns (finite, non-negative values only)"""
    u = to_float32(q).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def frames_from_native(flat, sizes, T, H, W, channels):
    """uint8 [clips, T, channels, H, W] of the ragged buffer flat (clip b's T frames of h0 w0 bytes, clip after clip), and the clips' offsets"""
    flat = np.asarray(flat)
    out = np.empty((len(sizes), T, channels, H, W), dtype=np.uint8)
    offs, off = [], 0
    for b, (h0, w0) in enumerate(sizes):
        offs.append(off)
        out[b] = area_bytes(flat[off:off + T * h0 * w0].reshape(T, h0, w0), H, W)[:, None]
        off += T * h0 * w0
    out.setflags(write=False)
    return out, offs


def pack(clips):
    """(flat uint8, sizes) of a list of [T, h0, w0] arrays"""
    return np.concatenate([np.asarray(c, dtype=np.uint8).reshape(-1) for c in clips]), [(int(c.shape[1]), int(c.shape[2])) for c in clips]
