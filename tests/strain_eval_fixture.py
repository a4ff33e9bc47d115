"""A small split with PRESCRIBED 4-class predictions for the comparison of eval.py's `strain` block and predict.segment_native's `strain` keys
with a restatement built on tests/contour_reference.py: 4 clips of 5 frames on a 32 x 32 grid (tests/contour_reference.heart_clip: a cavity
that shrinks and grows once, a wall around it, an atrium block that touches the cavity only while it is large), the prediction the same
drawing from another seed; clip 2 has no atrium on either side, so none of its frames has a base interface.  With batches of 3 the last
batch is short.  Test infrastructure: imports nothing from the product."""
import functools
import os

import numpy as np

from tests import contour_reference as R
from tests import eval_reference as ER
from tests import lv_reference as LV

CLIPS, T, H, W = 4, 5, 32, 32
NCLS, BATCH, CLS, WALL, BASE = 4, 3, 1, (2,), (3,)
NO_BASE = 2
SPACING = [(330, 468), (468, 330), (400, 400), (250, 610)]   # micrometres per pixel (row, column), one per clip


@functools.lru_cache(maxsize=None)
def build():
    """{"pred", "target": uint8 [CLIPS, T, H, W]}.  Deterministic; shared between the tests, never written."""
    target = np.stack([R.heart_clip(T, H, W, seed=b, with_atrium=b != NO_BASE) for b in range(CLIPS)])
    pred = np.stack([R.heart_clip(T, H, W, seed=100 + b, with_atrium=b != NO_BASE) for b in range(CLIPS)])
    for a in (pred, target):
        a.setflags(write=False)
    return {"pred": pred, "target": target}


def picks(clip, sp=None):
    """(ed, es) as the lv / lv_mm block picks them on the clip's own curve, or None when the clip has no EF"""
    n, v = ER.curves(clip, CLS, sp)
    idx, ref = LV.lv_ef_ref([v], [n])
    if idx[0][0] < 0 or not ref[0][0] > 0:
        return None
    return idx[0][0], idx[0][1]


def lengths(clip, sp=None):
    """(npix [T], [L_wall, L_base, L_axis] per frame) of one clip"""
    recs = [R.contour_ref(f, CLS, WALL, BASE, sp) for f in clip]
    return [r[0] for r in recs], [R.lengths_ref(r, sp) for r in recs]


def clip_strain(measured, target, sp=None):
    """{"gls": (pred, ref) or None, "axis": (pred, ref) or None} of one clip at the target's ED / ES; None where the clip does not count"""
    pk = picks(target, sp)
    if pk is None:
        return {"gls": None, "axis": None}
    out = {}
    (t_n, t_l), (p_n, p_l) = lengths(target, sp), lengths(measured, sp)
    for key, k in (("gls", 0), ("axis", 2)):
        ref = R.strain_ref([l[k] for l in t_l], t_n, *pk)
        got = R.strain_ref([l[k] for l in p_l], p_n, *pk)
        out[key] = (got[1], ref[1]) if ref[5] and got[5] else None
    if out["gls"] is None:
        out["axis"] = None
    return out


def block(mm=True, clip_range=None):
    """The `strain` block of the fixture as eval.py prints it"""
    fx = build()
    lo, hi = clip_range or (0, CLIPS)
    rows = [clip_strain(fx["pred"][b], fx["target"][b], SPACING[b] if mm else None) for b in range(lo, hi)]
    gls = [r["gls"] for r in rows if r["gls"] is not None]
    axis = [r["axis"] for r in rows if r["axis"] is not None]
    names = {"clips_with_ef": "clips_with_strain", "ef_mae": "gls_mae", "ef_bias": "gls_bias", "ef_pearson_r": "gls_pearson_r",
             "mean_ref_ef": "mean_ref_gls", "mean_pred_ef": "mean_pred_gls"}
    ax = {"clips_with_ef": "clips_with_landmarks", "ef_mae": "shortening_mae", "ef_bias": "shortening_bias", "ef_pearson_r": "shortening_pearson_r",
          "mean_ref_ef": "mean_ref_shortening", "mean_pred_ef": "mean_pred_shortening"}
    return {"unit": "mm" if mm else "px", "wall_classes": list(WALL), "base_classes": list(BASE),
            **{names[k]: ER.r5(v) for k, v in ER.compare(gls).items()},
            "long_axis": {**{ax[k]: ER.r5(v) for k, v in ER.compare(axis).items()}, "clips_without_landmarks": len(gls) - len(axis)}}


def write_split(root, split="val", spacing=True):
    """The fixture as an npy_clips tree: <root>/<split>/clip_XX.npz with `frames` [T, H, W] carrying the prescribed prediction's class index as
    the pixel value, `masks`, and (spacing=True) `spacing_um`."""
    fx = build()
    os.makedirs(os.path.join(root, split), exist_ok=True)
    for b in range(CLIPS):
        arrays = {"frames": fx["pred"][b], "masks": fx["target"][b]}
        if spacing:
            arrays["spacing_um"] = np.array(SPACING[b], np.int32)
        np.savez(os.path.join(root, split, f"clip_{b:02d}.npz"), **arrays)
    return root
