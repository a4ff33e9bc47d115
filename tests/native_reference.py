"""The rule of gdkvm_mask_to_native (include/gdkvm.h) restated in numpy int64 / Python integers, its counts, and eval.py's `native` block.
Imports nothing from the product: the tests compare the product with THIS."""
import numpy as np


def axis(n_out, n_in):
    """Per native index: the two clamped source indices and their weights (w0 + w1 = 2 n_out), int64."""
    o = np.arange(n_out, dtype=np.int64)
    num = (2 * o + 1) * n_in - n_out
    den = 2 * n_out
    i0 = num // den                                              # floor division: -1 in the first half-pixel
    f = num - i0 * den
    assert ((0 <= f) & (f < den)).all()
    return np.clip(i0, 0, n_in - 1), np.clip(i0 + 1, 0, n_in - 1), den - f, f


def votes(m, h0, w0, ncls):
    """int64 [ncls, h0, w0]: the votes of every class at every native pixel for the source frame m [H, W] uint8."""
    m = np.asarray(m)
    H, W = m.shape
    ya, yb, wya, wyb = axis(h0, H)
    xa, xb, wxa, wxb = axis(w0, W)
    v = np.zeros((ncls, h0, w0), np.int64)
    for ys, wy in ((ya, wya), (yb, wyb)):
        for xs, wx in ((xa, wxa), (xb, wxb)):
            src = m[ys][:, xs]
            w = wy[:, None] * wx[None, :]
            for c in range(ncls):
                v[c] += w * (src == c)
    return v


def labels(m, h0, w0, ncls):
    """out uint8 [h0, w0] alone (resize_labels without the tie map)."""
    v = votes(m, h0, w0, ncls)
    out = v.argmax(0).astype(np.uint8)
    out[v.max(0) == 0] = 255
    return out


def resize_labels(m, h0, w0, ncls):
    """(out uint8 [h0, w0], votes int64 [ncls, h0, w0], tie bool [h0, w0]): the class with the most votes, the smallest among equals (numpy's
    argmax returns the first), 255 where no class has a vote; tie = the two largest vote sums are equal (the pixels where another
    arithmetic may answer differently)."""
    v = votes(m, h0, w0, ncls)
    out = v.argmax(0).astype(np.uint8)
    out[v.max(0) == 0] = 255
    srt = np.sort(v, 0)
    return out, v, srt[-1] == srt[-2]


def nearest_labels(m, h0, w0):
    """Nearest neighbour at half-pixel centres (what bringing a mask back without the rule would do)."""
    m = np.asarray(m)
    H, W = m.shape
    yi = np.clip(np.round((np.arange(h0) + 0.5) * H / h0 - 0.5).astype(int), 0, H - 1)
    xi = np.clip(np.round((np.arange(w0) + 0.5) * W / w0 - 0.5).astype(int), 0, W - 1)
    return m[yi][:, xi]


def offsets(sizes, T):
    """([every clip's first byte], total bytes) of the ragged layout: clip b's T frames of h0 w0 bytes, clip b + 1 behind it."""
    offs, total = [], 0
    for h0, w0 in sizes:
        offs.append(total)
        total += T * int(h0) * int(w0)
    return offs, total


def pack(clips):
    """(flat uint8, sizes) of a list of [T, h0, w0] arrays."""
    return np.concatenate([np.asarray(c, np.uint8).reshape(-1) for c in clips]), [(c.shape[1], c.shape[2]) for c in clips]


def mask_to_native(mask, sizes, ncls, target=None):
    """(out flat uint8, counts int32 [clips, T, ncls, 3] or None) for mask [clips, T, H, W] uint8 and the flat target."""
    mask = np.asarray(mask)
    clips, T = mask.shape[:2]
    offs, total = offsets(sizes, T)
    out = np.empty(total, np.uint8)
    counts = np.zeros((clips, T, ncls, 3), np.int32) if target is not None else None
    for b, (h0, w0) in enumerate(sizes):
        for t in range(T):
            lo = offs[b] + t * h0 * w0
            o = labels(mask[b, t], h0, w0, ncls).reshape(-1)
            out[lo:lo + h0 * w0] = o
            if target is not None:
                g = np.asarray(target[lo:lo + h0 * w0])
                for c in range(ncls):
                    counts[b, t, c] = (int(((o == c) & (g == c)).sum()), int((o == c).sum()), int((g == c).sum()))
    return out, counts


def dice_iou(counts, eps=1e-6):
    """(Dice, IoU) per class from summed counts [ncls, 3], with eval.py's eps convention."""
    c = np.asarray(counts, np.float64)
    return (2.0 * c[:, 0] + eps) / (c[:, 1] + c[:, 2] + eps), (c[:, 0] + eps) / (c[:, 1] + c[:, 2] - c[:, 0] + eps)


def native_block(counts, sizes):
    """eval.py's `native` block from the per-frame counts [clips, T, ncls, 3] of every clip and the clips' sizes: a frame counts when its
    native target has a pixel of some class; pixels = the native pixels of those frames."""
    counts = np.asarray(counts, np.int64)
    lab = counts[..., 2].sum(-1) > 0                             # [clips, T]
    tot = (counts * lab[..., None, None]).sum((0, 1))
    d, i = dice_iou(tot)
    px = sum(int(lab[b].sum()) * int(h0) * int(w0) for b, (h0, w0) in enumerate(sizes))
    return {"dice_per_class": [round(float(v), 5) for v in d],
            "mean_foreground_dice": round(float(sum(d[1:]) / max(len(d) - 1, 1)), 5),
            "iou_per_class": [round(float(v), 5) for v in i],
            "mean_foreground_iou": round(float(sum(i[1:]) / max(len(i) - 1, 1)), 5),
            "pixels": px, "frames": int(lab.sum())}
