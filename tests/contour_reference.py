"""Reference of the contour record and its lengths (include/gdkvm.h, gdkvm_lv_contour; gdkvm_amd.ops.contour_lengths / lv_strain) in plain
Python / numpy: every word of the record is an exact Python integer, the lengths are Python floats (IEEE fp64, one rounding per operation) in
the order the definition gives.  Test infrastructure: imports nothing from the product."""
import math

import numpy as np

DIRS = ((0, 1), (1, 0), (1, 1), (1, -1))                    # E, S, SE, SW as (dy, dx)
BAND_ROWS, WORD_BITS = 64, 64                               # GDKVM_LV_CONTOUR_BAND_ROWS, GDKVM_LV_CONTOUR_WORD_BITS


def byte_set(members):
    s = 0
    for b in members:
        assert 0 <= int(b) <= 31
        s |= 1 << int(b)
    return s


def _in_set(padded, s):
    """bool array: the byte is below 32 and a member of the 32-bit set s"""
    lut = np.array([b < 32 and bool((s >> b) & 1) for b in range(256)])
    return lut[padded]


def contour_ref(mask, cls=1, wall=(2,), base=(3,), spacing=None):
    """One frame mask [H, W] (uint8) -> the 16 integers of its record.  spacing = (ry, rx) micrometres or None."""
    mask = np.asarray(mask, np.uint8)
    H, W = mask.shape
    ws, bs = byte_set(wall), byte_set(base)
    assert 1 <= H <= 1024 and 1 <= W <= 1024 and 0 <= cls <= 31 and ws and not (ws & bs) and not ((ws | bs) >> cls) & 1
    ry, rx = (1, 1) if spacing is None else (int(spacing[0]), int(spacing[1]))
    if not (1 <= ry <= 4095 and 1 <= rx <= 4095):
        return [-1] * 16
    padded = np.zeros((H + 2, W + 2), np.uint8)             # a position outside the frame reads as byte 0
    padded[1:-1, 1:-1] = mask
    ys, xs = np.nonzero(mask == cls)
    ys, xs = ys.astype(np.int64), xs.astype(np.int64)
    n = int(ys.size)
    counts, SX2, SY2 = [], 0, 0
    for which, s in enumerate((ws, bs)):
        member = _in_set(padded, s)
        for dy, dx in DIRS:
            fwd = member[ys + 1 + dy, xs + 1 + dx]          # the pair {p, p + d} with p of the class
            bwd = member[ys + 1 - dy, xs + 1 - dx]          # the pair {q - d, q} with q of the class
            counts.append(int(fwd.sum()) + int(bwd.sum()))
            if which == 1 and (dy, dx) in ((0, 1), (1, 0)):
                SX2 += int((2 * xs[fwd] + dx).sum()) + int((2 * xs[bwd] - dx).sum())
                SY2 += int((2 * ys[fwd] + dy).sum()) + int((2 * ys[bwd] - dy).sum())
    nb = counts[4] + counts[5]
    if nb == 0:
        return [n] + counts + [0, 0, -1, -1, -1, 0, 0]
    bx2, by2 = (2 * SX2 + nb) // (2 * nb), (2 * SY2 + nb) // (2 * nb)            # Python's // floors towards -infinity
    d2 = (ry * (2 * ys - by2)) ** 2 + (rx * (2 * xs - bx2)) ** 2                  # < 2^48
    best = int(d2.max())
    apex = int((ys * W + xs)[d2 == best].min())
    return [n] + counts + [SX2, SY2, bx2, by2, apex, best, 0]


def contour_ref_frames(frames, cls=1, wall=(2,), base=(3,), spacing=None):
    """frames [F, H, W] -> int64 [F, 16]; spacing None, one (ry, rx) for all, or [F, 2]"""
    frames = np.asarray(frames)
    sp = None if spacing is None else np.broadcast_to(np.asarray(spacing), (frames.shape[0], 2))
    return np.array([contour_ref(m, cls, wall, base, None if sp is None else sp[f]) for f, m in enumerate(frames)], dtype=np.int64).reshape(-1, 16)


def crofton_length(ne, ns, nse, nsw, ry=1, rx=1):
    """The Cauchy-Crofton length of four pair counts, in the spacing's unit (micrometres with a spacing, pixels at 1, 1)"""
    ry, rx = float(ry), float(rx)
    phi = math.atan2(ry, rx)
    delta = (ry * rx) / math.sqrt(ry * ry + rx * rx)
    return 0.5 * (phi * (float(ne) * ry) + (math.pi / 2 - phi) * (float(ns) * rx) + (math.pi / 4) * (float(nse + nsw) * delta))


def lengths_ref(rec, spacing=None):
    """[L_wall, L_base, L_axis] of one record: mm with a spacing (ry, rx) in micrometres, pixels without; -1 for a -1 record"""
    rec = [int(v) for v in rec]
    if rec[0] < 0:
        return [-1.0, -1.0, -1.0]
    ry, rx = (1, 1) if spacing is None else (int(spacing[0]), int(spacing[1]))
    unit = 1.0 if spacing is None else 1000.0
    return [crofton_length(*rec[1:5], ry, rx) / unit, crofton_length(*rec[5:9], ry, rx) / unit, math.sqrt(float(rec[14])) / 2.0 / unit]


def strain_ref(length, npix, ed, es, min_pixels=1):
    """One clip: (curve list, GLS, peak strain, L_ED, peak frame, ok) from the lists length and npix and the picked frames"""
    T = len(length)
    valid = [npix[t] >= min_pixels and length[t] > 0 for t in range(T)]
    ok = ed >= 0 and es >= 0 and valid[ed] and valid[es]
    if not ok:
        return [0.0] * T, 0.0, 0.0, 0.0, -1, False
    led = length[ed]
    curve = [(length[t] - led) / led if valid[t] else 0.0 for t in range(T)]
    peak, frame = None, -1
    for t in range(T):
        if valid[t] and (peak is None or curve[t] < peak):
            peak, frame = curve[t], t
    return curve, curve[es], peak, led, frame, True


# ------------------------------------------------------------------------------------------------------------------ shapes for the tests
def ellipse_labels(H, W, cy, cx, a, b, deg, inner=1, outer=2, ring=0.0, out=None):
    """Pixels whose centre lies inside the rotated ellipse of semi-axes a (along the direction deg from the x axis) and b become `inner`;
    with ring > 0 the pixels inside the ellipse scaled by 1 + ring that are not inner become `outer` first."""
    m = np.zeros((H, W), np.uint8) if out is None else out
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    t = math.radians(deg)
    u = (xx - cx) * math.cos(t) + (yy - cy) * math.sin(t)
    v = -(xx - cx) * math.sin(t) + (yy - cy) * math.cos(t)
    q = (u / a) ** 2 + (v / b) ** 2
    if ring > 0:
        m[q <= (1 + ring) ** 2] = outer
    m[q <= 1.0] = inner
    return m


def ellipse_perimeter(a, b, steps=20000):
    """The perimeter of an ellipse of semi-axes a, b: the complete elliptic integral by the midpoint rule (it converges geometrically for a
    periodic analytic integrand; 20000 steps are far below 1e-12)"""
    h = 2 * math.pi / steps
    return sum(math.hypot(a * math.sin((i + 0.5) * h), b * math.cos((i + 0.5) * h)) for i in range(steps)) * h


def heart_clip(T, H, W, seed=0, with_atrium=True):
    """A synthetic 4-class clip [T, H, W]: 0 background, 1 cavity (an ellipse that shrinks and grows once over the clip), 2 myocardium (a ring
    around it), 3 atrium: a block that cuts the lower end of the cavity off in every frame (with_atrium=True), none (False), or a block at
    a fixed height that the cavity reaches only near its largest size ("diastole": in systole the myocardium closes the gap, and those
    frames have a wall interface and no base interface)."""
    rng = np.random.default_rng(seed)
    cy, cx = H * 0.42 + rng.uniform(-1, 1), W * 0.5 + rng.uniform(-1, 1)
    out = np.zeros((T, H, W), np.uint8)
    for t in range(T):
        s = 1.0 - 0.22 * math.sin(math.pi * t / max(T - 1, 1)) ** 2
        a, b = H * 0.30 * s, W * 0.17 * s
        m = out[t]
        ellipse_labels(H, W, cy, cx, a, b, 90.0, inner=1, outer=2, ring=0.28, out=m)
        if with_atrium:
            top = int(round(cy + (H * 0.30 * 0.93 if with_atrium == "diastole" else a * 0.8)))
            blk = m[top:top + max(H // 6, 2), int(cx - W * 0.2):int(cx + W * 0.2) + 1]
            if with_atrium == "diastole":
                blk[blk != 1] = 3
            else:
                blk[...] = 3                                   # the mitral plane: a straight cut through the cavity
    return out
