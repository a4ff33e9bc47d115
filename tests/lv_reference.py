"""Reference of the left-ventricular measurement (include/gdkvm.h, gdkvm_lv_measure / gdkvm_lv_ef) in plain Python / numpy: every integer
quantity is an exact Python integer (numpy int64 is used only where the bounds below are asserted), the floating-point steps are Python floats
(IEEE fp64, no fused multiply-add) in the order the definition gives.  Test infrastructure: imports nothing from the product."""
import math

import numpy as np

Q = 1 << 16


def axis_from_moments(n, sx, sy, sxx, sxy, syy):
    """Step 3: (Ux, Uy), the eigenvector of the larger eigenvalue of the scaled central moments, in units of 1/Q."""
    A, B, C = n * sxx - sx * sx, n * sxy - sx * sy, n * syy - sy * sy
    a, b = float(A - C), float(2 * B)
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
    return int(round(ux * Q)), int(round(uy * Q))            # round(): half to even, as rint


def lv_measure_ref(mask, cls=1, D=20, axis=None):
    """One frame mask [H, W] (uint8).  Returns {"stats": 12 ints, "disks": D ints, "geom": [L, V, cx, cy]}.  axis = (Ux, Uy) overrides step 3
    (the device's own axis, or a fixed one for the rectangle KATs)."""
    mask = np.asarray(mask)
    H, W = mask.shape
    assert 1 <= H <= 1024 and 1 <= W <= 1024 and 1 <= D <= 64 and 0 <= cls <= 254
    ys, xs = np.nonzero(mask == cls)
    xs, ys = xs.astype(np.int64), ys.astype(np.int64)
    n = int(xs.size)
    if n == 0:
        return {"stats": [0] * 12, "disks": [0] * D, "geom": [0.0] * 4}
    sx, sy = int(xs.sum()), int(ys.sum())                    # < 2^30
    sxx, sxy, syy = int((xs * xs).sum()), int((xs * ys).sum()), int((ys * ys).sum())     # < 2^40
    Ux, Uy = axis if axis is not None else axis_from_moments(n, sx, sy, sxx, sxy, syy)
    assert abs(Ux) <= Q and abs(Uy) <= Q
    t = (n * xs - sx) * Ux + (n * ys - sy) * Uy              # |.| < 2^47 in int64
    tmin, tmax = int(t.min()), int(t.max())
    P1 = n * Q
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
    L = float(Lt) / float(P1)
    s = 0.0
    for w in disks:
        aj = float(w) / float(D * P1)
        s = s + aj * aj
    V = math.pi * D * s / (4.0 * L)
    stats = [n, sx, sy, sxx, sxy, syy, Ux, Uy, tmin, tmax, Lt, 0]
    return {"stats": stats, "disks": disks, "geom": [L, V, float(sx) / float(n), float(sy) / float(n)]}


def lv_ef_ref(vol, npix, pick_vol=None, pick_npix=None, min_pixels=1):
    """vol, npix [B, T] (and the optional pick arrays).  Returns (idx [B][3] = ed, es, nvalid; val [B][3] = EDV, ESV, EF)."""
    assert (pick_vol is None) == (pick_npix is None)
    pv = vol if pick_vol is None else pick_vol
    pn = npix if pick_npix is None else pick_npix
    idx, val = [], []
    for b in range(len(vol)):
        valid = [t for t in range(len(vol[b])) if int(pn[b][t]) >= min_pixels]
        if len(valid) < 2:
            idx.append([-1, -1, len(valid)])
            val.append([0.0, 0.0, 0.0])
            continue
        ed = es = valid[0]
        for t in valid[1:]:                                   # strict comparisons in ascending t: ties keep the lowest t
            if float(pv[b][t]) > float(pv[b][ed]):
                ed = t
            if float(pv[b][t]) < float(pv[b][es]):
                es = t
        edv, esv = float(vol[b][ed]), float(vol[b][es])
        idx.append([ed, es, len(valid)])
        val.append([edv, esv, 0.0 if edv == 0.0 else (edv - esv) / edv])
    return idx, val


def ellipse_mask(H, W, cy, cx, la, sa, deg, value=1, out=None):
    """Pixels whose centre lies inside the ellipse of semi-axes la (along the direction `deg` degrees from the image's vertical) and sa."""
    m = np.zeros((H, W), np.uint8) if out is None else out
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    th = math.radians(deg)
    dx, dy = xx - cx, yy - cy
    al = dx * math.sin(th) + dy * math.cos(th)
    ac = dx * math.cos(th) - dy * math.sin(th)
    m[(al / la) ** 2 + (ac / sa) ** 2 <= 1.0] = value
    return m
