"""The rule of gdkvm_overlay_native (include/gdkvm.h) restated in numpy from the header's text; shares no code with gdkvm_amd/ops.py.

A pixel is decided by the first case that applies: a contour pixel of the mask -> pal[k]; with a ref, a contour pixel of the ref ->
ref_pal[k']; a class byte k in the mask -> (g (256 - alpha) + pal[k][c] alpha + 128) >> 8 per channel; otherwise (g, g, g).  A contour pixel
holds a class byte (1 <= k < ncls) and has, within |dy| + |dx| <= w, a pixel outside the frame or one holding another byte."""
import numpy as np

# palettes the tests use where they do not mean the defaults: every channel of every class different, none of them a grey
PAL = np.array([[9, 8, 7], [250, 10, 20], [30, 240, 40], [50, 60, 230], [220, 210, 5], [200, 15, 190], [25, 180, 170], [255, 130, 3]], np.uint8)
REF_PAL = np.array([[1, 2, 3], [255, 254, 253], [245, 255, 200], [190, 250, 255], [252, 222, 251], [231, 232, 233], [210, 251, 212],
                    [249, 239, 219]], np.uint8)


def class_bytes(m, ncls):
    m = np.asarray(m)
    return (m >= 1) & (m < ncls)


def contour(m, ncls, w):
    """bool [h0, w0]: the contour pixels of the frame m, straight from the definition (a loop over the diamond, the frame's outside tested as
    such and not through a padding value)"""
    m = np.asarray(m, np.uint8)
    h0, w0 = m.shape
    yy, xx = np.mgrid[0:h0, 0:w0]
    differs = np.zeros((h0, w0), bool)
    for dy in range(-w, w + 1):
        for dx in range(-w, w + 1):
            if abs(dy) + abs(dx) > w or (dy == 0 and dx == 0):
                continue
            ny, nx = yy + dy, xx + dx
            outside = (ny < 0) | (ny >= h0) | (nx < 0) | (nx >= w0)
            other = m[np.clip(ny, 0, h0 - 1), np.clip(nx, 0, w0 - 1)] != m
            differs |= outside | other
    return class_bytes(m, ncls) & differs


def overlay_frame(g, m, r, ncls, w, alpha, pal=PAL, ref_pal=REF_PAL):
    """uint8 [h0, w0, 3] of one frame; r may be None"""
    g, m = np.asarray(g, np.uint8), np.asarray(m, np.uint8)
    pal, ref_pal = np.asarray(pal, np.int64), np.asarray(ref_pal, np.int64)
    out = np.repeat(g.astype(np.int64)[..., None], 3, -1)                                      # case 4
    inside = class_bytes(m, ncls)
    k = np.where(inside, m, 0).astype(np.int64)
    tint = (g.astype(np.int64)[..., None] * (256 - alpha) + pal[k] * alpha + 128) >> 8
    out[inside] = tint[inside]                                                                 # case 3
    if r is not None:
        r = np.asarray(r, np.uint8)
        on_r = contour(r, ncls, w)
        out[on_r] = ref_pal[r[on_r].astype(np.int64)]                                          # case 2
    on_m = contour(m, ncls, w)
    out[on_m] = pal[m[on_m].astype(np.int64)]                                                  # case 1
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def offsets(sizes, T):
    offs, total = [], 0
    for h0, w0 in sizes:
        offs.append(total)
        total += T * h0 * w0
    return offs, total


def pack(clips):
    """(flat uint8, sizes) of a list of [T, h0, w0] arrays: the ragged layout"""
    return np.concatenate([np.asarray(c, np.uint8).reshape(-1) for c in clips]), [(int(c.shape[1]), int(c.shape[2])) for c in clips]


def overlay_native(grey, mask, ref, sizes, T, ncls, w, alpha, pal=PAL, ref_pal=REF_PAL):
    """flat uint8 [3 total] from the ragged flat buffers grey, mask and ref (or None)"""
    offs, total = offsets(sizes, T)
    out = np.zeros(3 * total, np.uint8)
    for b, (h0, w0) in enumerate(sizes):
        for t in range(T):
            lo = offs[b] + t * h0 * w0
            fr = lambda a: a[lo:lo + h0 * w0].reshape(h0, w0)
            o = overlay_frame(fr(grey), fr(mask), None if ref is None else fr(ref), ncls, w, alpha, pal, ref_pal)
            out[3 * lo:3 * (lo + h0 * w0)] = o.reshape(-1)
    return out


def blobs(rng, T, h0, w0, ncls, stray=0.03):
    """A mask with structure at the scale of the contour widths: a coarse random class field enlarged by 1..4, then a sprinkle of single
    pixels of every byte the rule names (classes, bytes >= ncls, 254, 255)."""
    out = np.zeros((T, h0, w0), np.uint8)
    for t in range(T):
        s = int(rng.integers(1, 5))
        coarse = rng.integers(0, ncls, (-(-h0 // s), -(-w0 // s)))
        coarse[rng.random(coarse.shape) < 0.35] = 0
        out[t] = np.kron(coarse, np.ones((s, s), np.int64))[:h0, :w0]
    spr = rng.random(out.shape) < stray
    out[spr] = rng.choice(np.array([0, 1, ncls - 1, ncls, 8, 200, 254, 255], np.uint8), int(spr.sum()))
    return out
