"""A small split with PRESCRIBED predictions and native targets for the comparison of eval.py's `native` block with
tests/native_reference.native_block: 5 clips of 3 frames on a 32 x 32 grid with three classes (background, a cavity, a wall around it),
every clip with a native size of its own -- larger, smaller, squeezed either way, and equal to the grid.  The native target is drawn at the
native size, the grid target is its nearest-neighbour down-sampling (what a converter leaves), the prediction the same drawing a little off
on the grid; clip 1 carries an island of the cavity class in the prediction for the largest-component filter, and a pixel that flickers for
the temporal vote; clip 3 is labelled in its first frame only.  With batches of 2 the last batch is short.  Test infrastructure: imports
nothing from the product."""
import functools
import os

import numpy as np

from tests import eval_reference as ER
from tests import native_reference as R

CLIPS, T, H, W = 5, 3, 32, 32
NCLS, IGNORE, BATCH = 3, 255, 2
SIZES = [(47, 61), (32, 32), (70, 45), (21, 90), (55, 54)]
HALF_LABELLED = 3                                            # this clip's frames 1 and 2 carry no labels
ISLAND = 1
PARAMS = dict(num_classes=NCLS, lv_class=1, vote=0, keep=0, fill=0, fill_max_area=0)


def _drawing(h, w, cy, cx, ry, rx):
    y, x = np.mgrid[0:h, 0:w]
    d = (((y + 0.5) / h - cy) / ry) ** 2 + (((x + 0.5) / w - cx) / rx) ** 2
    m = np.zeros((h, w), np.uint8)
    m[d < 1.7] = 2
    m[d < 1.0] = 1
    return m


@functools.lru_cache(maxsize=None)
def build():
    """{"pred", "target": uint8 [CLIPS, T, H, W]; "native": a list of uint8 [T, h0, w0]}.  Deterministic; shared between the tests, never
    written."""
    pred, target, native = np.zeros((CLIPS, T, H, W), np.uint8), np.zeros((CLIPS, T, H, W), np.uint8), []
    for b, (h0, w0) in enumerate(SIZES):
        nat = np.zeros((T, h0, w0), np.uint8)
        for t in range(T):
            k = 1.0 - 0.08 * t
            nat[t] = _drawing(h0, w0, 0.5 + 0.02 * b, 0.47, 0.27 * k, (0.17 + 0.01 * b) * k)
            target[b, t] = R.nearest_labels(nat[t], H, W)
            pred[b, t] = _drawing(H, W, 0.51 + 0.02 * b, 0.45, 0.26 * k, (0.18 + 0.01 * b) * k)
        if b == ISLAND:
            pred[b, :, 2:5, 3:8] = 1                          # far from the cavity: the largest-component filter removes it
            pred[b, 1, 16, 16] = 0                            # one frame's pixel inside the cavity: the vote puts it back
        if b == HALF_LABELLED:
            nat[1:] = IGNORE
            target[b, 1:] = IGNORE
        native.append(nat)
    for a in [pred, target] + native:
        a.setflags(write=False)
    return {"pred": pred, "target": target, "native": native}


def block(clip_range=None, **over):
    """native_block of the fixture (the clips lo .. hi - 1 of clip_range) with PARAMS, `over` replacing single arguments; with a clean-up on,
    a "post" block of the post-processed prediction inside it, as eval.py prints it."""
    fx, p = build(), {**PARAMS, **over}
    lo, hi = clip_range or (0, CLIPS)
    flat, sizes = R.pack(fx["native"][lo:hi])
    out = R.native_block(R.mask_to_native(fx["pred"][lo:hi], sizes, NCLS, flat)[1], sizes)
    if p["vote"] or p["keep"] or p["fill"]:
        post = ER.post_process(fx["pred"][lo:hi], **p)["measured"]
        out["post"] = R.native_block(R.mask_to_native(post, sizes, NCLS, flat)[1], sizes)
    return out


def write_split(root, split="val", native=True):
    """The fixture as an npy_clips tree: <root>/<split>/clip_XX.npz with `frames` [T, H, W] carrying the prescribed prediction's class index as
    the pixel value, `masks` and (native=True) `native_target`; clip 2 goes without one with native="holes"."""
    fx = build()
    os.makedirs(os.path.join(root, split), exist_ok=True)
    for b in range(CLIPS):
        arrays = {"frames": fx["pred"][b], "masks": fx["target"][b]}
        if native is True or (native == "holes" and b != 2):
            arrays["native_target"] = fx["native"][b]
        np.savez(os.path.join(root, split, f"clip_{b:02d}.npz"), **arrays)
    return root
