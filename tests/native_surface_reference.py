"""Reference of the surface distances at native frame sizes (include/gdkvm.h, gdkvm_surface_distance_native) in numpy int64 and Python ints:
the definition restated for RAGGED clips -- every clip its own (h0, w0), each side in 1..2048, and its own spacing (ry, rx) in micrometres
per native pixel, each in 1..4095.  The surfaces are tests.surface_reference.surface; the exact squared distance transform is this file's own
(spacing_reference.edt2_um stops at sides of 1024), separable: vertical distances per column, then a minimum over the row; math.isqrt for
the fixed-point sums.  Also the eval report's native.surface block from such records.  Test infrastructure: imports nothing from the product
and needs no scipy."""
import math

import numpy as np

from tests.surface_reference import surface

SIDE_MAX, UM_MAX = 2048, 4095
_FAR = 1 << 62                                               # "no surface pixel in this column": above every real squared distance (< 2^47)


def edt2_um(Sf, ry, rx):
    """int64 [h0, w0]: the squared distance in um^2 from every pixel to the nearest True pixel of Sf, (ry dy)^2 + (rx dx)^2 (>= 2^62 when Sf
    is empty).  Exact: every term is below 2^46."""
    Sf = np.asarray(Sf, bool)
    H, W = Sf.shape
    assert 1 <= ry <= UM_MAX and 1 <= rx <= UM_MAX and 1 <= H <= SIDE_MAX and 1 <= W <= SIDE_MAX
    big = 1 << 20
    ys = np.arange(H, dtype=np.int64)[:, None]
    last = np.maximum.accumulate(np.where(Sf, ys, -big), axis=0)
    nxt = np.minimum.accumulate(np.where(Sf, ys, big)[::-1], axis=0)[::-1]
    g = np.minimum(ys - last, nxt - ys)
    g2 = np.where(g >= big // 2, _FAR, (g * ry) ** 2)
    xs = np.arange(W, dtype=np.int64)
    dx2 = ((xs[:, None] - xs[None, :]) * rx) ** 2            # [x, x']
    out = np.empty((H, W), np.int64)
    for y in range(H):
        out[y] = (dx2 + g2[y][None, :]).min(axis=1)
    return out


def _fixed_sum(d2):
    vals, cnt = np.unique(d2, return_counts=True)
    return sum(math.isqrt(int(v) << 16) * int(c) for v, c in zip(vals, cnt))


def frame_record(mask, target, ry, rx, cls=1):
    """One native frame -> the record of 8 Python ints: nA, nB, hAB, hBA (um^2), sAB, sBA (2^-8 um), q_lo, q_hi (um^2)."""
    mask, target = np.asarray(mask), np.asarray(target)
    assert mask.dtype == np.uint8 and target.dtype == np.uint8 and mask.shape == target.shape and mask.ndim == 2 and 0 <= cls <= 254
    SA, SB = surface(mask == cls), surface(target == cls)
    nA, nB = int(SA.sum()), int(SB.sum())
    if nA == 0 or nB == 0:
        return [nA, nB, 0, 0, 0, 0, 0, 0]
    dab, dba = edt2_um(SB, ry, rx)[SA], edt2_um(SA, ry, rx)[SB]
    pooled = np.sort(np.concatenate([dab, dba]))
    n = nA + nB
    lo = (95 * (n - 1)) // 100
    hi = min(lo + 1, n - 1)
    return [nA, nB, int(dab.max()), int(dba.max()), _fixed_sum(dab), _fixed_sum(dba), int(pooled[lo]), int(pooled[hi])]


def records(masks, targets, spacing, cls=1):
    """masks, targets: lists of uint8 [T, h0, w0], one per clip; spacing [clips][2] -> int64 [clips, T, 8].  Frames are independent."""
    assert len(masks) == len(targets) == len(spacing)
    return np.asarray([[frame_record(m[t], g[t], int(s[0]), int(s[1]), cls) for t in range(m.shape[0])]
                       for m, g, s in zip(masks, targets, spacing)], np.int64).reshape(len(masks), -1, 8)


def pack(clips):
    """(flat uint8, sizes) of a list of [T, h0, w0]: clip b's frames follow each other, clip b + 1 follows clip b."""
    return np.concatenate([np.ascontiguousarray(c).reshape(-1) for c in clips]), [(int(c.shape[1]), int(c.shape[2])) for c in clips]


def metrics_mm(rec):
    """(HD, HD95, ASSD in mm, valid) of one record as Python floats: the definition of ops.surface_metrics_mm."""
    nA, nB, hAB, hBA, sAB, sBA, q_lo, q_hi = (int(v) for v in rec)
    if nA <= 0 or nB <= 0:
        return 0.0, 0.0, 0.0, False
    a, b = math.sqrt(q_lo) / 1000, math.sqrt(q_hi) / 1000
    return math.sqrt(max(hAB, hBA)) / 1000, a + (b - a) * (((95 * (nA + nB - 1)) % 100) / 100), (sAB / nA + sBA / nB) / 2 / 256 / 1000, True


def surface_block(recs, counted, cls, unit, digits=5):
    """The report's native.surface block from records [frames, 8] and `counted` [frames] (the native target of the frame has a pixel of the
    class): the frames with both surfaces are averaged, those with exactly one are reported."""
    n = one = 0
    hd = hd95 = assd = 0.0
    for rec, c in zip(np.asarray(recs).reshape(-1, 8), np.asarray(counted).reshape(-1)):
        if not c:
            continue
        a, b, s, valid = metrics_mm(rec)
        if valid:
            n, hd, hd95, assd = n + 1, hd + a, hd95 + b, assd + s
        elif (rec[0] > 0) != (rec[1] > 0):
            one += 1
    d = max(n, 1)
    return {"class": int(cls), "unit": unit, "frames": n, "frames_one_empty": one, "hd_mean": round(hd / d, digits),
            "hd95_mean": round(hd95 / d, digits), "assd_mean": round(assd / d, digits)}
