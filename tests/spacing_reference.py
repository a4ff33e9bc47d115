"""Reference of the measurements with a pixel spacing (include/gdkvm.h, gdkvm_surface_distance_mm / gdkvm_lv_measure_mm) in numpy integers,
Python ints and Python floats: the exact squared distance transform in micrometres, math.isqrt for the fixed-point sums, and the left-
ventricular measurement with its axis found in the physical plane, the floating-point steps in the order the definition gives (IEEE fp64, no
fused multiply-add).  A spacing is (ry, rx): micrometres per pixel down the rows and along the columns, each in 1..4095.  Test infrastructure:
imports nothing from the product and needs no scipy."""
import math

import numpy as np

from tests import surface_reference as S

Q = 1 << 16
UM_MAX = 4095
_FAR = 1 << 62                                               # "no surface pixel in this column": above every real squared distance (< 2^45)


def edt2_um(Sf, ry, rx):
    """int64 [H, W]: the squared distance in um^2 from every pixel to the nearest True pixel of Sf, (ry dy)^2 + (rx dx)^2 (>= 2^62 when Sf is
    empty).  Exact: every term is below 2^45."""
    Sf = np.asarray(Sf, bool)
    H, W = Sf.shape
    assert 1 <= ry <= UM_MAX and 1 <= rx <= UM_MAX and H <= 1024 and W <= 1024
    big = 1 << 20
    ys = np.arange(H, dtype=np.int64)[:, None]
    last = np.maximum.accumulate(np.where(Sf, ys, -big), axis=0)
    nxt = np.minimum.accumulate(np.where(Sf, ys, big)[::-1], axis=0)[::-1]
    g = np.minimum(ys - last, nxt - ys)
    g2 = np.where(g >= big // 2, _FAR, (g * ry) ** 2)        # a column without a surface pixel offers nothing
    xs = np.arange(W, dtype=np.int64)
    dx2 = ((xs[:, None] - xs[None, :]) * rx) ** 2            # [x, x']
    out = np.empty((H, W), np.int64)
    for y in range(H):
        out[y] = (dx2 + g2[y][None, :]).min(axis=1)
    return out


def _fixed_sum(d2):
    vals, cnt = np.unique(d2, return_counts=True)
    return sum(math.isqrt(int(v) << 16) * int(c) for v, c in zip(vals, cnt))


def surface_distance_mm_ref(mask, target, ry, rx, cls=1):
    """One frame -> the record of 8 Python ints: nA, nB, hAB, hBA (um^2), sAB, sBA (2^-8 um), q_lo, q_hi (um^2); eight -1 for a spacing out of
    range."""
    if not (1 <= ry <= UM_MAX and 1 <= rx <= UM_MAX):
        return [-1] * 8
    mask, target = np.asarray(mask), np.asarray(target)
    assert mask.dtype == np.uint8 and target.dtype == np.uint8 and mask.shape == target.shape and mask.ndim == 2 and 0 <= cls <= 254
    SA, SB = S.surface(mask == cls), S.surface(target == cls)
    nA, nB = int(SA.sum()), int(SB.sum())
    if nA == 0 or nB == 0:
        return [nA, nB, 0, 0, 0, 0, 0, 0]
    dab, dba = edt2_um(SB, ry, rx)[SA], edt2_um(SA, ry, rx)[SB]
    pooled = np.sort(np.concatenate([dab, dba]))
    n = nA + nB
    lo = (95 * (n - 1)) // 100
    hi = min(lo + 1, n - 1)
    return [nA, nB, int(dab.max()), int(dba.max()), _fixed_sum(dab), _fixed_sum(dba), int(pooled[lo]), int(pooled[hi])]


def surface_distance_mm_frames(mask, target, spacing, cls=1):
    """[F, H, W], spacing [F][2] (or one pair for all) -> int64 [F, 8]."""
    sp = np.broadcast_to(np.asarray(spacing, np.int64), (mask.shape[0], 2))
    return np.asarray([surface_distance_mm_ref(mask[f], target[f], int(sp[f, 0]), int(sp[f, 1]), cls) for f in range(mask.shape[0])],
                      np.int64).reshape(-1, 8)


def metrics_mm_ref(rec):
    """(HD, HD95, ASSD in mm, valid) of one record as Python floats: the definition of ops.surface_metrics_mm."""
    nA, nB, hAB, hBA, sAB, sBA, q_lo, q_hi = (int(v) for v in rec)
    if nA <= 0 or nB <= 0:
        return 0.0, 0.0, 0.0, False
    a, b = math.sqrt(q_lo) / 1000, math.sqrt(q_hi) / 1000
    return math.sqrt(max(hAB, hBA)) / 1000, a + (b - a) * (((95 * (nA + nB - 1)) % 100) / 100), (sAB / nA + sBA / nB) / 2 / 256 / 1000, True


def axis_mm_from_moments(n, sx, sy, sxx, sxy, syy, ry, rx):
    """Step 3': (Vx, Vy, E, k) -- the long axis in the physical plane in units of 1/Q of the larger reduced spacing, one pixel's extent along
    it in the same units, and that extent in micrometres."""
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
    Vx = int(round((ux * float(px * Q)) / float(pm)))        # round(): half to even, as rint
    Vy = int(round((uy * float(py * Q)) / float(pm)))
    E = int(round((e * float(Q)) / float(pm)))
    return Vx, Vy, E, e * float(g)


def lv_measure_mm_ref(mask, ry, rx, cls=1, D=20, axis=None):
    """One frame mask [H, W] (uint8) -> {"stats": 12 ints = n sx sy sxx sxy syy Vx Vy tmin tmax Lt E, "disks": D ints, "geom": [L mm, V mL,
    cx mm, cy mm, k um, area mm^2]}.  axis = (Vx, Vy, E, k) overrides step 3' (the device's own axis, or a fixed one).  A spacing out of
    range gives -1 everywhere, an empty frame 0."""
    mask = np.asarray(mask)
    H, W = mask.shape
    assert 1 <= H <= 1024 and 1 <= W <= 1024 and 1 <= D <= 64 and 0 <= cls <= 254
    if not (1 <= ry <= UM_MAX and 1 <= rx <= UM_MAX):
        return {"stats": [-1] * 12, "disks": [-1] * D, "geom": [-1.0] * 6}
    ys, xs = np.nonzero(mask == cls)
    xs, ys = xs.astype(np.int64), ys.astype(np.int64)
    n = int(xs.size)
    if n == 0:
        return {"stats": [0] * 12, "disks": [0] * D, "geom": [0.0] * 6}
    sx, sy = int(xs.sum()), int(ys.sum())
    sxx, sxy, syy = int((xs * xs).sum()), int((xs * ys).sum()), int((ys * ys).sum())
    Vx, Vy, E, k = axis if axis is not None else axis_mm_from_moments(n, sx, sy, sxx, sxy, syy, ry, rx)
    assert abs(Vx) <= Q and abs(Vy) <= Q and 16 <= E <= Q
    t = (n * xs - sx) * Vx + (n * ys - sy) * Vy              # |.| < 2^47 in int64
    tmin, tmax = int(t.min()), int(t.max())
    P1 = n * E
    Lt = tmax - tmin + P1
    assert D * Lt < 1 << 62
    lo = D * (t - tmin)
    hi = lo + D * P1
    disks = []
    for j in range(D):
        ov = np.minimum(hi, (j + 1) * Lt) - np.maximum(lo, j * Lt)
        ov = np.where(ov > 0, ov, 0)
        assert int(ov.max()) * n < 1 << 63
        disks.append(int(ov.sum()))
    L = ((float(Lt) / float(P1)) * k) / 1000.0
    pix = float(ry * rx) / 1e6
    s = 0.0
    for w in disks:
        aj = (float(w) / float(D * P1)) * pix
        s = s + aj * aj
    V = ((math.pi * D) * s) / (4.0 * L) / 1000.0
    geom = [L, V, ((float(sx) / float(n)) * float(rx)) / 1000.0, ((float(sy) / float(n)) * float(ry)) / 1000.0, k, float(n * ry * rx) / 1e6]
    return {"stats": [n, sx, sy, sxx, sxy, syy, Vx, Vy, tmin, tmax, Lt, E], "disks": disks, "geom": geom}
