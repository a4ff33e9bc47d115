"""Reference of gdkvm_lv_measure_native (include/gdkvm.h) in numpy int64, Python ints and Python floats: steps 1, 2, 3', 4, 5 and 6' of
gdkvm_lv_measure_mm on a native frame with sides up to 2048, the floating-point steps in the order the definition gives (IEEE fp64, no fused
multiply-add), A, B and C in Python integers.  Every bound the header states for the integer widths is ASSERTED on every input, and the
per-band rows (the entry's `bands` output) are returned beside the records.  Test infrastructure: imports nothing from the product."""
import math

import numpy as np

Q = 1 << 16
UM_MAX = 4095
MAX_SIDE = 2048
BAND_ROWS = 32                                               # GDKVM_LV_NATIVE_BAND_ROWS
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)


def axis(n, sx, sy, sxx, sxy, syy, ry, rx):
    """Steps 2 and 3': (Vx, Vy, E, k) from Python integers; |A|, |B|, |C| < 2^63 asserted."""
    g = math.gcd(ry, rx)
    py, px = ry // g, rx // g
    pm = max(px, py)
    A, B, C = n * sxx - sx * sx, n * sxy - sx * sy, n * syy - sy * sy
    assert 0 <= A < 1 << 63 and 0 <= C < 1 << 63 and abs(B) < 1 << 63, (A, B, C)
    assert A == (n * sxx - sx * sx) % (1 << 64) and C == (n * syy - sy * sy) % (1 << 64)        # the wrap-around difference is the value
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


def measure(mask, ry, rx, cls=1, D=20, axis_override=None):
    """One native frame [h0, w0] uint8 -> {"stats": 12 ints, "disks": D ints, "geom": 6 floats, "bands": [nbands][8 + D] ints}.
    axis_override = (Vx, Vy, E, k): the device's own axis in place of step 3'."""
    mask = np.asarray(mask)
    h0, w0 = mask.shape
    assert mask.dtype == np.uint8 and 1 <= h0 <= MAX_SIDE and 1 <= w0 <= MAX_SIDE and 1 <= D <= 64 and 0 <= cls <= 254
    assert 1 <= ry <= UM_MAX and 1 <= rx <= UM_MAX
    nbands = (h0 + BAND_ROWS - 1) // BAND_ROWS
    ys, xs = np.nonzero(mask == cls)
    xs, ys = xs.astype(np.int64), ys.astype(np.int64)
    n = int(xs.size)
    if n == 0:
        return {"stats": [0] * 12, "disks": [0] * D, "geom": [0.0] * 6, "bands": [[0] * (8 + D) for _ in range(nbands)]}
    present, starts = np.unique(ys // BAND_ROWS, return_index=True)      # (np.nonzero walks row-major: the bands' pixels are runs)

    def per_band(v, op=np.add, fill=0):
        out = np.full(nbands, fill, np.int64)
        out[present] = op.reduceat(v, starts)
        return out

    mom = [per_band(v) for v in (np.ones_like(xs), xs, ys, xs * xs, xs * ys, ys * ys)]
    tot = [int(v.sum()) for v in mom]
    sx, sy = tot[1], tot[2]
    assert n <= 1 << 22 and sx < 1 << 33 and sy < 1 << 33 and max(tot[3:]) < 1 << 44
    Vx, Vy, E, k = axis_override if axis_override is not None else axis(*tot, ry, rx)
    assert abs(Vx) <= Q and abs(Vy) <= Q and 16 <= E <= Q
    assert int(np.abs(n * xs - sx).max()) < 1 << 33 and int(np.abs(n * ys - sy).max()) < 1 << 33
    t = (n * xs - sx) * Vx + (n * ys - sy) * Vy
    assert int(np.abs(t).max()) < 1 << 50
    b_min, b_max = per_band(t, np.minimum, I64_MAX), per_band(t, np.maximum, I64_MIN)
    tmin, tmax = int(t.min()), int(t.max())
    P1 = n * E
    Lt = tmax - tmin + P1
    assert P1 <= 1 << 38 and Lt < (1 << 51) + (1 << 38)
    lo = D * (t - tmin)
    hi = lo + D * P1
    assert int(hi.max()) < 1 << 58 and D * Lt < 1 << 58
    w_band, disks = [], []
    for j in range(D):
        ov = np.minimum(hi, (j + 1) * Lt) - np.maximum(lo, j * Lt)
        ov = np.where(ov > 0, ov, 0)
        assert int(ov.max()) <= D * P1
        # W_j exactly, in Python integers: the halves' sums are below 2^32 2^22; the band sums are parts of it, so they cannot wrap either
        disks.append((int((ov >> 32).sum()) << 32) + int((ov & 0xffffffff).sum()))
        assert disks[-1] < 1 << 63
        w_band.append(per_band(ov))
        assert disks[-1] == sum(int(v) for v in w_band[-1])
    assert sum(disks) == n * D * P1
    L = ((float(Lt) / float(P1)) * k) / 1000.0
    pix = float(ry * rx) / 1e6
    s = 0.0
    for w in disks:
        aj = (float(w) / float(D * P1)) * pix
        s = s + aj * aj
    V = ((math.pi * D) * s) / (4.0 * L) / 1000.0
    geom = [L, V, ((float(sx) / float(n)) * float(rx)) / 1000.0, ((float(sy) / float(n)) * float(ry)) / 1000.0, k, float(n * ry * rx) / 1e6]
    rows = np.stack(mom + [b_min, b_max] + w_band, 1)
    return {"stats": tot + [Vx, Vy, tmin, tmax, Lt, E], "disks": disks, "geom": geom, "bands": [[int(v) for v in r] for r in rows]}


def pack(clips):
    """[T, h0, w0] uint8 arrays -> (the ragged flat uint8 array, [(h0, w0), ...])"""
    return (np.concatenate([np.ascontiguousarray(c).reshape(-1) for c in clips]) if clips else np.zeros(0, np.uint8),
            [tuple(int(v) for v in c.shape[1:]) for c in clips])


def records(clips, spacing, cls=1, D=20, axes=None):
    """(stats int64 [clips, T, 12], disks int64 [clips, T, D], geom float64 [clips, T, 6], bands int64 [native_bands, 8 + D]) for clips of
    equal T.  axes[b][t] = (Vx, Vy, E, k) or None overrides step 3' per frame."""
    T = clips[0].shape[0]
    st, dk, ge, rows = [], [], [], []
    for b, c in enumerate(clips):
        for t in range(T):
            r = measure(c[t], int(spacing[b][0]), int(spacing[b][1]), cls, D, None if axes is None else axes[b][t])
            st.append(r["stats"]); dk.append(r["disks"]); ge.append(r["geom"]); rows += r["bands"]
    return (np.asarray(st, np.int64).reshape(len(clips), T, 12), np.asarray(dk, np.int64).reshape(len(clips), T, D),
            np.asarray(ge, np.float64).reshape(len(clips), T, 6), np.asarray(rows, np.int64).reshape(-1, 8 + D))
