"""Reference of the largest-connected-component filter (include/gdkvm.h, gdkvm_largest_component) in plain Python / numpy: a union-find over the
pixels of the class (no sweep-until-unchanged loop: a serpentine would take H W / 2 sweeps), exact integers throughout.  Test infrastructure:
imports nothing from the product and needs no scipy."""
import numpy as np


def label_components(mask, cls=1, connectivity=4):
    """labels int64 [H, W]: the smallest linear index y W + x of the pixel's component for pixels of `cls`, -1 elsewhere."""
    mask = np.asarray(mask)
    H, W = mask.shape
    assert 1 <= H <= 1024 and 1 <= W <= 1024 and 0 <= cls <= 254 and connectivity in (4, 8)
    flat = (mask == cls).ravel()
    inp = flat.tolist()
    parent = list(range(H * W))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    def union(a, b):
        a, b = find(a), find(b)
        if a < b:
            parent[b] = a
        elif b < a:
            parent[a] = b

    idx = np.flatnonzero(flat).tolist()
    for p in idx:                                            # backward neighbours only: every adjacent pair is met once, from its later pixel
        y, x = divmod(p, W)
        if x > 0 and inp[p - 1]:
            union(p, p - 1)
        if y > 0:
            if inp[p - W]:
                union(p, p - W)
            if connectivity == 8:
                if x > 0 and inp[p - W - 1]:
                    union(p, p - W - 1)
                if x < W - 1 and inp[p - W + 1]:
                    union(p, p - W + 1)
    labels = np.full(H * W, -1, np.int64)
    for p in idx:
        labels[p] = find(p)                                  # the smaller root always wins a union: a root is its component's smallest index
    return labels.reshape(H, W)


def largest_component_ref(mask, cls=1, connectivity=4, fill=0, target=None):
    """One frame mask [H, W] (uint8), optional target [H, W].  Returns (out uint8 [H, W], info = 8 Python ints)."""
    mask = np.asarray(mask)
    assert mask.dtype == np.uint8 and 0 <= fill <= 255 and fill != cls
    labels = label_components(mask, cls, connectivity)
    lab = labels[labels >= 0]
    n = int(lab.size)
    if n == 0:
        return mask.copy(), [0, 0, 0, -1, 0, 0, 0, 0]
    names, sizes = np.unique(lab, return_counts=True)        # names ascend: argmax returns the FIRST maximum, the smallest label of a tie
    k = int(np.argmax(sizes))
    kept, n_kept = int(names[k]), int(sizes[k])
    removed = (labels >= 0) & (labels != kept)
    out = mask.copy()
    out[removed] = fill
    hit_cls = hit_fill = 0
    if target is not None:
        t = np.asarray(target)
        assert t.shape == mask.shape
        hit_cls, hit_fill = int((t[removed] == cls).sum()), int((t[removed] == fill).sum())
    assert int(removed.sum()) == n - n_kept
    return out, [int(names.size), n, n_kept, kept, hit_cls, hit_fill, 0, 0]


def largest_component_frames(frames, cls=1, connectivity=4, fill=0, target=None):
    """frames [F, H, W] -> (out [F, H, W], info int32 [F, 8]): the frames are independent."""
    outs, infos = [], []
    for f in range(frames.shape[0]):
        o, i = largest_component_ref(frames[f], cls, connectivity, fill, None if target is None else target[f])
        outs.append(o)
        infos.append(i)
    return np.stack(outs), np.asarray(infos, np.int32).reshape(-1, 8)


def counts_ref(mask, target, ncls):
    """argmax_dice-style counts int64 [ncls, 3] = |A n B|, |A|, |B| of one or more frames."""
    mask, target = np.asarray(mask), np.asarray(target)
    return np.asarray([[int(((mask == c) & (target == c)).sum()), int((mask == c).sum()), int((target == c).sum())] for c in range(ncls)], np.int64)


# ---- shapes that the definition's corners need ----------------------------------------------------------------------------------------------
def serpentine(H, W, cls=1):
    """Full even rows, one pixel in every odd row alternately at the right and the left end: ONE 4-connected component whose longest path
    runs through every pixel (64 x 64: 32 * 64 + 32 = 2080 pixels; with an even H the last row's pixel is a stub)."""
    m = np.zeros((H, W), np.uint8)
    m[0::2, :] = cls
    for k, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = cls
    return m


def spiral(H, W, cls=1):
    """A rectangular spiral of one-pixel walls and one-pixel gaps from the frame's corner inwards: one 4-connected component."""
    m = np.zeros((H, W), np.uint8)
    free = lambda yy, xx: 0 <= yy < H and 0 <= xx < W and m[yy, xx] == 0
    wall = lambda yy, xx: 0 <= yy < H and 0 <= xx < W and m[yy, xx] == cls
    y, x, dy, dx, turns = 0, 0, 0, 1, 0
    m[0, 0] = cls
    while turns < 2:
        if free(y + dy, x + dx) and not wall(y + 2 * dy, x + 2 * dx):
            y, x, turns = y + dy, x + dx, 0
            m[y, x] = cls
        else:
            dy, dx, turns = dx, -dy, turns + 1              # turn right; two turns without a step: the centre is reached
    return m


def checkerboard(H, W, cls=1):
    m = np.zeros((H, W), np.uint8)
    m[(np.add.outer(np.arange(H), np.arange(W)) % 2) == 0] = cls
    return m


def disc(m, cy, cx, r, value=1):
    yy, xx = np.mgrid[0:m.shape[0], 0:m.shape[1]]
    m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = value
    return m
