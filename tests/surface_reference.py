"""Reference of the surface distances (include/gdkvm.h, gdkvm_surface_distance) in numpy integers and Python ints: the surfaces by shifted
comparisons, the exact squared Euclidean distance transform separably (vertical distances per column, then a minimum over the row), math.isqrt
for the fixed-point sums.  Also the mask builders the surface tests share.  Test infrastructure: imports nothing from the product and needs
no scipy."""
import math

import numpy as np

from tests import cc_reference as C
from tests import lv_reference as R

_BIG = 1 << 20                                               # "no surface pixel in this column": BIG^2 is above every real squared distance


def surface(X):
    """The pixels of the boolean set X [H, W] with a 4-neighbour outside X; outside the frame is outside X."""
    X = np.asarray(X, bool)
    P = np.pad(X, 1, constant_values=False)
    inner = P[:-2, 1:-1] & P[2:, 1:-1] & P[1:-1, :-2] & P[1:-1, 2:]
    return X & ~inner


def edt2(S):
    """int64 [H, W]: the squared Euclidean distance from every pixel to the nearest True pixel of S (>= BIG^2 when S is empty)."""
    S = np.asarray(S, bool)
    H, W = S.shape
    ys = np.arange(H, dtype=np.int64)[:, None]
    last = np.maximum.accumulate(np.where(S, ys, -_BIG), axis=0)             # the nearest surface row at or above y, per column
    nxt = np.minimum.accumulate(np.where(S, ys, _BIG)[::-1], axis=0)[::-1]   # ... at or below y
    g = np.minimum(np.minimum(ys - last, nxt - ys), _BIG)
    g2 = g * g
    xs = np.arange(W, dtype=np.int64)
    dx2 = (xs[:, None] - xs[None, :]) ** 2                                   # [x, x']
    out = np.empty((H, W), np.int64)
    for y in range(H):
        out[y] = (dx2 + g2[y][None, :]).min(axis=1)
    return out


def directed(mask, target, cls=1):
    """(S(A), S(B), d2_AB at S(A), d2_BA at S(B)) for one frame; the d2 arrays are int64 in row-major order of the surface pixels and empty when
    either surface is."""
    mask, target = np.asarray(mask), np.asarray(target)
    assert mask.dtype == np.uint8 and target.dtype == np.uint8 and mask.shape == target.shape and mask.ndim == 2
    assert 1 <= mask.shape[0] <= 1024 and 1 <= mask.shape[1] <= 1024 and 0 <= cls <= 254
    SA, SB = surface(mask == cls), surface(target == cls)
    if not SA.any() or not SB.any():
        return SA, SB, np.zeros(0, np.int64), np.zeros(0, np.int64)
    return SA, SB, edt2(SB)[SA], edt2(SA)[SB]


def _fixed_sum(d2):
    vals, cnt = np.unique(d2, return_counts=True)
    return sum(math.isqrt(int(v) << 32) * int(c) for v, c in zip(vals, cnt))


def surface_distance_ref(mask, target, cls=1):
    """One frame -> the record of 8 Python ints: nA, nB, hAB, hBA, sAB, sBA, q_lo, q_hi."""
    SA, SB, dab, dba = directed(mask, target, cls)
    nA, nB = int(SA.sum()), int(SB.sum())
    if nA == 0 or nB == 0:
        return [nA, nB, 0, 0, 0, 0, 0, 0]
    pooled = np.sort(np.concatenate([dab, dba]))
    n = nA + nB
    lo = (95 * (n - 1)) // 100
    hi = min(lo + 1, n - 1)
    return [nA, nB, int(dab.max()), int(dba.max()), _fixed_sum(dab), _fixed_sum(dba), int(pooled[lo]), int(pooled[hi])]


def surface_distance_frames(mask, target, cls=1):
    """[F, H, W] -> int64 [F, 8]: the frames are independent."""
    return np.asarray([surface_distance_ref(mask[f], target[f], cls) for f in range(mask.shape[0])], np.int64).reshape(-1, 8)


def metrics_ref(rec):
    """(HD, HD95, ASSD, valid) of one record as Python floats: the definition of ops.surface_metrics."""
    nA, nB, hAB, hBA, sAB, sBA, q_lo, q_hi = (int(v) for v in rec)
    if nA == 0 or nB == 0:
        return 0.0, 0.0, 0.0, False
    a, b = math.sqrt(q_lo), math.sqrt(q_hi)
    return math.sqrt(max(hAB, hBA)), a + (b - a) * ((95 * (nA + nB - 1)) % 100) / 100, (sAB / nA + sBA / nB) / 2 / 65536, True


# ---- the masks the tests share ---------------------------------------------------------------------------------------------------------------
def random_frames(F, H, W, seed):
    """Unions of random rotated ellipses of classes 1 and 2, speckle of both, a patch of class 3 and one of 255 (the recipe of the LV test)."""
    rng = np.random.default_rng(seed)
    out = np.zeros((F, H, W), np.uint8)
    for f in range(F):
        m = out[f]
        for value in (2, 1, 1):
            la = rng.uniform(0.12, 0.4) * max(H, W)
            sa = rng.uniform(0.08, 0.3) * min(H, W)
            R.ellipse_mask(H, W, rng.uniform(0.3, 0.7) * H, rng.uniform(0.3, 0.7) * W, la, sa, rng.uniform(0, 180), value=value, out=m)
        sp = rng.random((H, W))
        m[sp < 0.004] = 1
        m[sp > 0.996] = 2
        m[: max(H // 8, 1), : max(W // 5, 1)] = 3
        m[H - max(H // 9, 1):, W // 2:] = 255
    return out


def run_frames(F, H, W, seed):
    """Frames for shapes too thin for ellipses (a single row or column, a few pixels across): random runs of 1 to 6 pixels along the rows,
    of classes 0, 1, 2, 3 and 255, redrawn until classes 1 and 2 both occur in every frame."""
    rng = np.random.default_rng(seed)
    out = np.zeros((F, H, W), np.uint8)
    values = np.asarray([0, 1, 2, 1, 2, 0, 3, 255], np.uint8)
    for f in range(F):
        for _ in range(100):
            flat, p = np.zeros(H * W, np.uint8), 0
            while p < H * W:
                n = int(rng.integers(1, 7))
                flat[p:p + n] = values[int(rng.integers(0, len(values)))]
                p += n
            if (flat == 1).any() and (flat == 2).any():
                break
        else:
            raise AssertionError(f"run_frames: no frame of {H} x {W} with classes 1 and 2")
        out[f] = flat.reshape(H, W)
    return out


def lattice(H, W, cls=1):
    """Every pixel of the class except those with (x + 2 y) mod 5 == 0: each hole has four neighbours of the class and no two holes share
    one, so 4/5 of the frame is surface."""
    m = np.full((H, W), cls, np.uint8)
    m[(np.add.outer(2 * np.arange(H), np.arange(W)) % 5) == 0] = 0
    return m


def special_pairs(H, W, cls):
    """(mask, target) frames at the definition's corners (degenerate but valid on the one-pixel-wide shapes)."""
    z = lambda: np.zeros((H, W), np.uint8)
    full = lambda: np.full((H, W), cls, np.uint8)
    one = lambda y, x: (lambda m: (m.__setitem__((y, x), cls), m)[1])(z())
    blob = z()
    blob[H // 4: max(3 * H // 4, H // 4 + 1), W // 4: max(3 * W // 4, W // 4 + 1)] = cls
    pairs = [(z(), blob), (blob, z()), (z(), z()),                           # each of the three empty cases
             (blob, blob.copy()),                                            # A == B
             (full(), one(H // 2, W // 2)), (one(H // 2, W // 2), full()),   # the full frame against one pixel
             (one(0, 0), one(H - 1, W - 1)), (one(H - 1, 0), one(0, W - 1)), # opposite corners: the largest d2 this shape has
             (C.checkerboard(H, W, cls), np.roll(C.checkerboard(H, W, cls), 1, 1) if W > 1 else blob),      # every pixel of the class is surface
             (C.checkerboard(H, W, cls), blob),
             (lattice(H, W, cls), one(H - 1, 0)), (blob, lattice(H, W, cls))]                                # 4/5 of the frame is surface
    m, t = z(), z()                                                          # one-pixel-wide lines
    m[H // 3, :] = cls; m[:, W // 3] = cls
    t[(2 * H) // 3, :] = cls; t[:, W - 1] = cls
    pairs.append((m, t))
    m, t = z(), z()                                                          # (W - 1, y) beside (0, y + 1) in memory: no neighbours
    m[:, W - 1] = cls; m[:, 0] = cls
    t[0, W - 1] = cls; t[min(1, H - 1), 0] = cls
    pairs.append((m, t))
    m, t = z(), z()                                                          # the last byte of this frame ...
    m[H - 1, W - 1] = cls; t[0, 0] = cls; t[H - 1, W - 1] = cls
    pairs.append((m, t))
    m, t = z(), z()                                                          # ... and the first byte of the next
    m[0, 0] = cls; t[0, 0] = cls; m[H - 1, W - 1] = cls
    pairs.append((m, t))
    m, t = np.full((H, W), 255, np.uint8), np.full((H, W), 255 - cls, np.uint8)      # other bytes are not the class
    m[H // 2, W // 2] = cls; t[0, W - 1] = cls
    pairs.append((m, t))
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def case_frames(F, H, W, cls):
    """(mask, target) uint8 [F + specials, H, W]: random frames against other random frames, then the special pairs."""
    a, b = random_frames(F, H, W, seed=H * 1000 + W), random_frames(F, H, W, seed=H * 1000 + W + 7)
    sm, st = special_pairs(H, W, cls)
    return np.concatenate([a, sm]), np.concatenate([b, st])
