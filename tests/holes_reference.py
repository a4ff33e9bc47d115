"""Reference of the hole filling (include/gdkvm.h, gdkvm_fill_holes) in plain Python / numpy: cc_reference's union-find over the COMPLEMENT of the
class, a component being outside when it holds a pixel of the frame's border, exact integers throughout.  Test infrastructure: imports nothing
from the product and needs no scipy."""
import numpy as np

from tests import cc_reference as C


def hole_labels(mask, cls=1, connectivity=4):
    """(labels int64 [H, W], sizes {label: pixels}): the smallest linear index of the pixel's HOLE (a component of the complement of `cls`,
    `connectivity` that of the complement, without a pixel on the frame's border), -1 for every other pixel."""
    mask = np.asarray(mask)
    H, W = mask.shape
    comp = (mask != cls).astype(np.uint8)
    labels = C.label_components(comp, 1, connectivity)
    border = np.concatenate([labels[0], labels[-1], labels[:, 0], labels[:, -1]])
    outside = np.unique(border[border >= 0])
    labels = np.where(np.isin(labels, outside), -1, labels)
    names, counts = np.unique(labels[labels >= 0], return_counts=True)
    return labels, {int(k): int(v) for k, v in zip(names, counts)}


def fill_holes_ref(mask, cls=1, connectivity=4, max_area=0, target=None):
    """One frame mask [H, W] (uint8), optional target [H, W].  Returns (out uint8 [H, W], info = 8 Python ints: holes, holes_filled, n, filled,
    largest_hole, hit_before, hit_filled, n_target)."""
    mask = np.asarray(mask)
    assert mask.dtype == np.uint8 and 0 <= cls <= 254 and max_area >= 0
    labels, sizes = hole_labels(mask, cls, connectivity)
    chosen = [k for k, s in sizes.items() if max_area == 0 or s <= max_area]
    fill = np.isin(labels, chosen) if chosen else np.zeros(mask.shape, bool)
    out = mask.copy()
    out[fill] = cls
    n, filled = int((mask == cls).sum()), int(fill.sum())
    assert filled == sum(sizes[k] for k in chosen) and not (fill & (mask == cls)).any()
    hit_before = hit_filled = n_target = 0
    if target is not None:
        t = np.asarray(target)
        assert t.shape == mask.shape
        hit_before, hit_filled, n_target = int((t[mask == cls] == cls).sum()), int((t[fill] == cls).sum()), int((t == cls).sum())
    return out, [len(sizes), len(chosen), n, filled, max(sizes.values(), default=0), hit_before, hit_filled, n_target]


def fill_holes_frames(frames, cls=1, connectivity=4, max_area=0, target=None):
    """frames [F, H, W] -> (out [F, H, W], info int32 [F, 8]): the frames are independent."""
    outs, infos = [], []
    for f in range(frames.shape[0]):
        o, i = fill_holes_ref(frames[f], cls, connectivity, max_area, None if target is None else target[f])
        outs.append(o)
        infos.append(i)
    return np.stack(outs), np.asarray(infos, np.int32).reshape(-1, 8)


# ---- hand-drawn frames: one per corner of the definition, drawn in a 13 x 13 corner of a frame of any larger shape ----------------------------
def hand_frames(H, W, cls=1):
    """{name: frame [H, W]} with H, W >= 13; every other pixel is 0 (or 2 when cls == 0)."""
    assert H >= 13 and W >= 13
    bg = 2 if cls == 0 else 0
    z = lambda: np.full((H, W), bg, np.uint8)
    fr = {}
    m = z(); m[1:6, 1:6] = cls; m[2:5, 2:5] = bg; m[1, 1] = bg                 # the ring's corner pixel is missing: the hole leaks diagonally
    fr["diagonal leak"] = m
    m = z(); m[1:7, 1:7] = cls; m[2:4, 2:4] = bg; m[4:6, 4:6] = bg             # two 2 x 2 holes that touch at one corner
    fr["diagonal holes"] = m
    m = z(); m[0:5, 2:7] = cls; m[0:3, 4] = bg                                 # a notch open to the frame's edge
    fr["notch"] = m
    m = z(); m[0, :] = cls; m[H - 1, :] = cls; m[:, 0] = cls; m[:, W - 1] = cls  # the class along the whole border
    fr["border frame"] = m
    m = z(); m[1:12, 1:12] = cls; m[2:11, 2:11] = bg; m[4:9, 4:9] = cls; m[6, 6] = bg   # a hole inside an island inside a hole
    fr["nested"] = m
    m = z(); m[1:12, 1:12] = cls; m[4:9, 4:9] = bg; m[2, 2] = bg; m[2, 9:11] = bg; m[10, 3] = bg   # a ring: a 25-pixel cavity, speckle of 1, 2, 1
    fr["ring"] = m
    m = z(); m[1:8, 1:8] = cls; m[2:7, 2:7] = 255; m[3, 3] = 3; m[4, 4] = 2 if cls != 2 else 0; m[5, 5] = 0 if cls != 0 else 7
    fr["other bytes"] = m
    return fr


def plugged_spiral(H, W, cls=1):
    """The class everywhere but for a one-pixel spiral corridor of 0 from (1, 1) inwards (cc_reference.spiral inside a one-pixel margin of the
    class, which plugs its outer end): ONE hole whose longest path runs through every one of its pixels."""
    assert H >= 5 and W >= 5 and cls != 0
    m = np.full((H, W), cls, np.uint8)
    m[1:H - 1, 1:W - 1][C.spiral(H - 2, W - 2, 1) == 1] = 0
    return m
