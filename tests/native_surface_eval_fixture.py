"""The split of tests/native_eval_fixture.py (its build(): prescribed predictions, native targets of five sizes) with a spacing of the NATIVE
pixel per clip, for the comparison of eval.py's native.surface block with tests/native_surface_reference.surface_block.  Written as an
npy_clips tree whose .npz carry `native_spacing_um`; the tree without them is native_eval_fixture.write_split's.  Test infrastructure: imports
nothing from the product."""
import os

import numpy as np

from tests import native_eval_fixture as F
from tests import native_reference as R
from tests import native_surface_reference as NR

CLS = 1
SPACING = [(308, 154), (300, 300), (154, 308), (471, 333), (1, 4095)]     # micrometres per native pixel, one anisotropy per clip
assert len(SPACING) == F.CLIPS


def write_split(root, split="val", spacing=True):
    """native_eval_fixture's tree (frames = the prescribed class index, masks, native_target) with `native_spacing_um` in every clip's .npz
    (spacing=True), in none (False), or in all but clip 2 ("holes")."""
    fx = F.build()
    os.makedirs(os.path.join(root, split), exist_ok=True)
    for b in range(F.CLIPS):
        arrays = {"frames": fx["pred"][b], "masks": fx["target"][b], "native_target": fx["native"][b]}
        if spacing is True or (spacing == "holes" and b != 2):
            arrays["native_spacing_um"] = np.asarray(SPACING[b], np.int32)
        np.savez(os.path.join(root, split, f"clip_{b:02d}.npz"), **arrays)
    return root


def block(clip_range=None, unit="mm", cls=CLS):
    """The native.surface block of the clips lo .. hi - 1: the RAW prediction taken to every clip's native size (native_reference's rule)
    against the native target, over the frames whose native target has a pixel of some class; unit "px" measures at 1000 x 1000 um."""
    fx = F.build()
    lo, hi = clip_range or (0, F.CLIPS)
    flat, sizes = R.pack(fx["native"][lo:hi])
    out, counts = R.mask_to_native(fx["pred"][lo:hi], sizes, F.NCLS, flat)
    offs, _ = R.offsets(sizes, F.T)
    pred = [out[o:o + F.T * h0 * w0].reshape(F.T, h0, w0) for o, (h0, w0) in zip(offs, sizes)]
    sp = SPACING[lo:hi] if unit == "mm" else [(1000, 1000)] * (hi - lo)
    recs = NR.records(pred, [np.asarray(n) for n in fx["native"][lo:hi]], sp, cls)
    counted = np.asarray(counts, np.int64)[..., 2].sum(-1) > 0
    return NR.surface_block(recs, counted, cls, unit)
