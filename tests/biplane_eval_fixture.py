"""A small split of patients' views with PRESCRIBED predictions for the comparison of eval.py's `biplane` block with
tests/biplane_reference.biplane_block_ref: 7 clips of 4 frames of 64 x 64 with two classes -- a patient with a 2CH view only, then three
patients with both views, so that with batches of 2 every pair straddles two batches.  The target of a view is an ellipse that shrinks from
end-diastole to end-systole, the prediction the same drawing a little off; clips 2 and 5 carry an island of class 1 in the prediction for the
largest-component filter; the 4CH target of the last patient is labelled in one frame only, so that pair has no target curve; per clip a
spacing of its own, and per clip what the files state: both views of the first pair (the values differ), the 4CH view only of the second (an
EF and no volumes), none for the third.  Test infrastructure: imports nothing from the product."""
import functools
import json

import numpy as np

from tests import biplane_reference as R

CLIPS, T, H, W = 7, 4, 64, 64
IGNORE = 255
BATCH = 2
PATIENTS = ["patient0001", "patient0002", "patient0002", "patient0003", "patient0003", "patient0004", "patient0004"]
VIEWS = ["2CH", "2CH", "4CH", "2CH", "4CH", "2CH", "4CH"]
PAIRS = [(1, 2), (3, 4), (5, 6)]
ISLANDS = (2, 5)
UNLABELLED = (6, 2)                                          # clip 6's target is labelled in this frame only
INFO = [{"ef_percent": 50.0, "edv_ml": 1.0, "esv_ml": 0.5},
        {"ef_percent": 41.5, "edv_ml": 0.52, "esv_ml": 0.31, "ed_frame": 1, "es_frame": 4, "nb_frame": 4, "frame_rate": None},
        {"ef_percent": 43.0, "edv_ml": 0.55, "esv_ml": None},
        None,
        {"ef_percent": 36.0, "edv_ml": None, "esv_ml": None},
        None,
        None]
PARAMS = dict(num_classes=2, lv_class=1, keep=0, fill=0, fill_max_area=0, vote=0)


@functools.lru_cache(maxsize=None)
def build():
    """{"pred", "target": uint8 [CLIPS, T, H, W]; "spacing": int32 [CLIPS, 2]}.  Deterministic; shared between the tests, never written."""
    pred, target = np.zeros((CLIPS, T, H, W), np.uint8), np.zeros((CLIPS, T, H, W), np.uint8)
    spacing = np.asarray([[300 + 29 * b, 270 + 31 * ((b * 3) % 7)] for b in range(CLIPS)], np.int32)
    for b in range(CLIPS):
        c, s, th = 7.0 + 0.25 * b, 2.6 + 0.3 * (b % 3), 0.12 - 0.05 * b
        for t in range(T):
            kt, kp = 1.0 - (0.07 + 0.01 * b) * t, 1.0 - (0.06 + 0.012 * ((b * 2) % 5)) * t
            target[b, t] = R.ellipse_view(H, W, *spacing[b], c * kt, s * kt, th, cy_mm=0.2 * b - 0.6, cx_mm=0.5 - 0.15 * b)
            pred[b, t] = R.ellipse_view(H, W, *spacing[b], 0.97 * c * kp, 1.04 * s * kp, th + 0.03, cy_mm=0.2 * b - 0.4, cx_mm=0.4 - 0.15 * b)
        if b in ISLANDS:                                     # far from the ventricle, towards a corner: it stretches the long axis
            pred[b, :, 2:5, 3 + b:7 + b] = 1
    target[UNLABELLED[0], [t for t in range(T) if t != UNLABELLED[1]]] = IGNORE
    for a in (pred, target, spacing):
        a.setflags(write=False)
    return {"pred": pred, "target": target, "spacing": spacing}


def block(clip_range=None, **over):
    """biplane_block_ref of the fixture with PARAMS, `over` replacing single arguments."""
    fx = build()
    return R.biplane_block_ref(fx["pred"], fx["target"], clip_range=clip_range,
                               **{**PARAMS, "spacing": fx["spacing"], "patients": PATIENTS, "views": VIEWS, "info": INFO, **over})


def as_dataset_arrays(spacing=True):
    """What tests/biplane_eval_driver.py reads: frames uint8 [CLIPS, T, 3, H, W] carrying the prediction's class index as the pixel value of
    every channel, the target, the names and one JSON text per clip."""
    fx = build()
    frames = np.ascontiguousarray(np.broadcast_to(fx["pred"][:, :, None], (CLIPS, T, 3, H, W)))
    out = {"frames": frames, "target": fx["target"], "patients": np.asarray(PATIENTS), "views": np.asarray(VIEWS),
           "info": np.asarray([json.dumps(i) for i in INFO])}
    if spacing:
        out["spacing"] = fx["spacing"]
    return out
