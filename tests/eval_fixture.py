"""A small split with PRESCRIBED predictions for the comparison of eval.py's report with tests/eval_reference.py: 7 clips of 24 frames of
64 x 64 with three classes -- a breathing ellipse of class 1 (three end-systoles per clip) inside a ring of class 2 as the target, and as the
prediction the same drawing a little off, with flicker for the temporal vote, islands for the largest-component filter, holes small and large
for the fill, a stretch without the class, frames without the ring -- and per clip a spacing, a length and a file EF of its own.
fixture_conditions states, with the references only, the facts that make the comparison worth its time (something to vote, filter and fill;
unlabelled, padded and dropped clips; batches that differ), so that a test can assert them before it trusts a match.  Test infrastructure:
imports nothing from the product."""
import functools
import math

import numpy as np

from tests import beats_reference as BT
from tests import eval_reference as E
from tests import holes_reference as HO
from tests import lv_reference as LV
from tests import surface_reference as SF

CLIPS, T, H, W = 7, 24, 64, 64
IGNORE = 255
# run A of the GPU test: everything on.  batch_size 2 over 7 clips: three full batches and a short one, through a prefetcher of 3 slots
PARAMS = dict(num_classes=3, lv_class=1, keep=4, fill=4, fill_max_area=6, vote=1, surface_class=2, lv_beats=True, beat_distance=4, beat_permille=500)
BATCH = 2
PERIOD = 8.0                                                 # frames per beat: end-systoles near frames 4, 12 and 20
VANISH = (2, range(9, 14))                                   # clip 2's prediction holds no class 1 in these frames: longer than the vote's window
SHORT = (3, 17)                                              # clip 3 has 17 frames of its own; the end-systole near frame 20 is padding
HALF = 4                                                     # clip 4's target labels the even frames only
SINGLE = (5, 7)                                              # clip 5's target labels this frame only


def _draw(cy, cx, la, sa, deg, ring=True):
    m = np.zeros((H, W), np.uint8)
    if ring:
        LV.ellipse_mask(H, W, cy, cx, la + 5.0, sa + 4.0, deg, value=2, out=m)
    return LV.ellipse_mask(H, W, cy, cx, la, sa, deg, value=1, out=m)


@functools.lru_cache(maxsize=None)
def build(seed=20):
    """{"pred", "target": uint8 [CLIPS, T, H, W]; "spacing": int32 [CLIPS, 2] (row_um, col_um); "lengths": int32 [CLIPS]; "file_ef": float64
    [CLIPS], per cent or NaN}.  Deterministic; the arrays are shared between the tests and must not be written."""
    rng = np.random.default_rng(seed)
    pred, target = np.zeros((CLIPS, T, H, W), np.uint8), np.zeros((CLIPS, T, H, W), np.uint8)
    for b in range(CLIPS):
        cy, cx = 31.3 + 0.9 * b - 2.0, 32.6 - 0.7 * b + 1.5
        la0, sa0, deg = 17.0 + 0.45 * b, 10.0 + 0.35 * (b % 4), 8.0 + 6.5 * b
        amp_t, amp_p = 0.11 + 0.015 * b, 0.10 + 0.022 * ((b * 3) % 7)      # the breathing of target and prediction: one EF per clip, each
        t0 = 3.6 + 0.13 * b                                                # the first end-systole
        for t in range(T):
            s = math.cos(2.0 * math.pi * (t - t0) / PERIOD)                # -1 at end-diastole ... 1 at end-systole
            target[b, t] = _draw(cy, cx, la0 * (1.0 - amp_t * s), sa0 * (1.0 - amp_t * s), deg,
                                 ring=not (b == 6 and t in (2, 3)))        # two target frames without the ring
            pred[b, t] = _draw(cy + 0.7, cx - 0.4, 0.96 * la0 * (1.0 - amp_p * s), 1.03 * sa0 * (1.0 - amp_p * s), deg + 2.0,
                               ring=not (b == 1 and 5 <= t <= 8))          # four predicted frames without it
        iy, ix = int(round(cy)), int(round(cx))
        if b in (0, 3, 6):                                   # an island of class 1 outside the ring in some frames
            pred[b, 6:16, 3:5, 4 + b:7 + b] = 1
        if b in (0, 4):                                      # holes of 1 and 2 pixels in every frame
            pred[b, :, iy - 3, ix - 2] = 0
            pred[b, :, iy + 2, ix + 1:ix + 3] = 2
        if b in (1, 3):                                      # a hole of 9 pixels: above fill_max_area
            pred[b, :, iy - 1:iy + 2, ix - 1:ix + 2] = 0
        if b in (3, 6):                                      # a hole of 4
            pred[b, :, iy + 4:iy + 6, ix - 3:ix - 1] = 0
        if b != 5:                                           # flicker: pixels redrawn in one frame only
            for t in range(T):
                ys, xs = rng.integers(0, H, 14), rng.integers(0, W, 14)
                pred[b, t, ys, xs] = rng.integers(0, 3, 14, dtype=np.uint8)
    # clip 1's large hole with one of its three rows closed in turn, frame by frame: a hole of 6 the fill would take in every single frame,
    # but no closing pixel lasts, so the vote reopens all 9 and the fill, which comes after it, leaves them -- the order of the chain shows
    iy, ix = int(round(31.3 + 0.9 - 2.0)), int(round(32.6 - 0.7 + 1.5))
    pred[1, :, iy - 1:iy + 2, ix - 1:ix + 2] = 0
    for t in range(T):
        pred[1, t, iy - 1 + t % 3, ix - 1:ix + 2] = 1
    pred[VANISH[0], VANISH[1].start:VANISH[1].stop][pred[VANISH[0], VANISH[1].start:VANISH[1].stop] == 1] = 0
    target[HALF, 1::2] = IGNORE
    target[SINGLE[0], [t for t in range(T) if t != SINGLE[1]]] = IGNORE
    spacing = np.asarray([[310 + 37 * b, 275 + 23 * ((b * 5) % 7)] for b in range(CLIPS)], np.int32)
    lengths = np.full(CLIPS, T, np.int32)
    lengths[SHORT[0]] = SHORT[1]
    file_ef = np.asarray([55.0, np.nan, 48.0, 61.5, np.nan, 40.0, 52.0])
    for a in (pred, target, spacing, lengths, file_ef):
        a.setflags(write=False)
    return {"pred": pred, "target": target, "spacing": spacing, "lengths": lengths, "file_ef": file_ef}


def report(fx=None, **over):
    """eval_report_ref of the fixture with PARAMS, `over` replacing single arguments (spacing, lengths, file_ef, pred, target included)."""
    fx = dict(build() if fx is None else fx)
    fx.update({k: over.pop(k) for k in list(over) if k in fx})
    return E.eval_report_ref(fx["pred"], fx["target"], spacing=fx["spacing"], lengths=fx["lengths"], file_ef=fx["file_ef"], **{**PARAMS, **over})


def tie_distance(masks, cls, spacing=None):
    """The smallest distance from a rounding tie (k + 1/2) of the unrounded long-axis components of every non-empty frame of masks [clips, T,
    H, W]: ux Q and uy Q of lv_reference.axis_from_moments, or with a spacing table Vx, Vy and E of spacing_reference.axis_mm_from_moments
    (the same expressions, in the same order, up to the rounding)."""
    Q, best = float(LV.Q), 0.5
    for b in range(masks.shape[0]):
        for f in masks[b]:
            ys, xs = np.nonzero(f == cls)
            n = int(xs.size)
            if n == 0:
                continue
            xs, ys = xs.astype(np.int64), ys.astype(np.int64)
            sx, sy, sxx, sxy, syy = int(xs.sum()), int(ys.sum()), int((xs * xs).sum()), int((xs * ys).sum()), int((ys * ys).sum())
            A, B, C = n * sxx - sx * sx, n * sxy - sx * sy, n * syy - sy * sy
            if spacing is None:
                px = py = pm = 1
            else:
                g = math.gcd(int(spacing[b][0]), int(spacing[b][1]))
                py, px = int(spacing[b][0]) // g, int(spacing[b][1]) // g
                pm = max(px, py)
            a, bb = float(px * px) * float(A) - float(py * py) * float(C), 2.0 * (float(px * py) * float(B))
            r = math.sqrt(a * a + bb * bb)
            vx, vy = (0.0, 1.0) if r == 0.0 else (a + r, bb) if a >= 0.0 else (bb, r - a)
            nrm = math.sqrt(vx * vx + vy * vy)
            ux, uy = vx / nrm, vy / nrm
            if spacing is None:
                vals = [ux * Q, uy * Q]
            else:
                ex, ey = ux * float(px), uy * float(py)
                vals = [(ux * float(px * LV.Q)) / float(pm), (uy * float(py * LV.Q)) / float(pm), (math.sqrt(ex * ex + ey * ey) * Q) / float(pm)]
            best = min([best] + [abs(abs(v) % 1.0 - 0.5) for v in vals])
    return best


def fixture_conditions(fx=None, params=None):
    """The facts a comparison on this fixture rests on, computed with the references only: a dict of numbers and booleans whose meaning the
    keys and the comments say.  tests/test_eval_report_cpu.py asserts every one."""
    fx = build() if fx is None else fx
    p = dict(PARAMS if params is None else params)
    pred, target, spacing, lengths = fx["pred"], fx["target"], fx["spacing"], fx["lengths"]
    ncls, cls, B = p["num_classes"], p["lv_class"], pred.shape[0]
    st = E.post_process(pred, num_classes=ncls, lv_class=cls, vote=p["vote"], keep=p["keep"], fill=p["fill"], fill_max_area=p["fill_max_area"])
    voted, filtered, filled = st["voted"], st["filtered"], st["filled"]
    lab = E.labelled_frames(target, ncls)
    f = {}
    # the vote, the filter and the fill all have work, and not everywhere
    f["clips_the_vote_changes"] = int(((voted != pred).sum((1, 2, 3)) > 0).sum())
    removed = ((voted == cls) & (filtered != cls)).sum((2, 3))
    f["frames_filtered"], f["frames_not_filtered"] = int((removed > 0).sum()), int((removed == 0).sum())
    f["pixels_filled"] = int(((filled == cls) & (filtered != cls)).sum())
    f["holes_left_above_max_area"] = sum(1 for b in range(B) for t in range(T)
                                         for s in HO.hole_labels(filled[b, t], cls, p["fill"])[1].values()
                                         if s > p["fill_max_area"] > 0)
    # a fill that moves the volume at one of the target's ED / ES frames
    moved = 0
    for b in range(B):
        t_n, t_v = E.curves(target[b], cls)
        idx, _ = LV.lv_ef_ref([t_v], [t_n])
        for t in idx[0][:2]:
            if t >= 0 and LV.lv_measure_ref(filtered[b, t], cls)["geom"][1] != LV.lv_measure_ref(filled[b, t], cls)["geom"][1]:
                moved += 1
    f["ed_es_volumes_the_fill_moves"] = moved
    # batches: a short last one, four at least (the prefetcher has 3 slots and results are collected one batch behind)
    f["clips_mod_batch"], f["batches"] = B % BATCH, -(-B // BATCH)
    # spacings: one per clip, all numbers distinct, none isotropic
    f["distinct_spacing_values"] = len({int(v) for v in spacing.reshape(-1)})
    f["isotropic_spacings"] = int((spacing[:, 0] == spacing[:, 1]).sum())
    # EF: who has one, and how the values spread
    efs = {b: E.clip_ef(st["measured"][b], target[b], cls) for b in range(B)}
    have = [b for b in range(B) if efs[b] is not None]
    f["clips_with_ef"] = len(have)
    f["distinct_pred_ef"], f["distinct_ref_ef"] = len({efs[b][0][2] for b in have}), len({efs[b][1][2] for b in have})
    f["batches_of_equal_ef"] = sum(1 for k in range(0, B - 1, BATCH) if all(efs[b] is not None for b in (k, k + 1)) and efs[k][0][2] == efs[k + 1][0][2])
    f["ef_pearson_r"] = E.compare([(efs[b][0][2], efs[b][1][2]) for b in have])["ef_pearson_r"]
    f["clips_with_one_labelled_frame"] = int((lab.sum(1) == 1).sum())
    f["single_frame_clip_has_ef"] = efs[SINGLE[0]] is not None
    # the clip labelled in every second frame: the prediction holds the class where the target says nothing
    f["half_clip_labelled_frames"] = int(lab[HALF].sum())
    f["half_clip_pred_pixels_in_unlabelled_frames"] = int((pred[HALF][~lab[HALF]] == cls).sum())
    # the surface class: every kind of frame
    s_cls = p["surface_class"]
    recs = np.stack([SF.surface_distance_frames(pred[b], target[b], s_cls) for b in range(B)])
    both, one = (recs[..., 0] > 0) & (recs[..., 1] > 0), (recs[..., 0] > 0) != (recs[..., 1] > 0)
    f["surface_frames_both"], f["surface_frames_one_empty"], f["surface_frames_unlabelled"] = int((both & lab).sum()), int((one & lab).sum()), int((~lab).sum())
    # beats
    args = dict(distance=p["beat_distance"], permille=p["beat_permille"])
    beats = []
    for b in range(B):
        area, vol = E.curves(st["measured"][b], cls, spacing[b])
        _, _, (info,), _ = BT.lv_beats_ref([area], [vol], [int(lengths[b])], **args)
        _, _, (whole,), _ = BT.lv_beats_ref([area], [vol], [T], **args)
        beats.append((info, whole, area))
    f["clips_with_two_beats"] = sum(1 for info, _, _ in beats if info[2] == 0 and info[0] >= 2)
    gap = [t for t in range(T) if beats[VANISH[0]][2][t] == 0]
    f["vanished_frames_after_the_chain"], f["vote_window"] = len(gap), 2 * p["vote"] + 1
    f["vanished_clip_is_dropped"] = beats[VANISH[0]][0][2] > 0
    f["short_clip_length"] = int(lengths[SHORT[0]])
    f["short_clip_systoles"], f["short_clip_systoles_with_padding"] = beats[SHORT[0]][0][1], beats[SHORT[0]][1][1]
    full = [bool(lab[b, :int(lengths[b])].all()) for b in range(B)]
    f["clips_the_target_covers"], f["clips_it_does_not"] = sum(full), B - sum(full)
    f["file_ef_nan"], f["file_ef_numbers"] = int(np.isnan(fx["file_ef"]).sum()), int((~np.isnan(fx["file_ef"])).sum())
    # axis rounding: how near any measured frame comes to a tie, in pixels and in the physical plane
    f["tie_distance"] = min(tie_distance(m, cls, sp) for m in (st["measured"], target) for sp in (None, spacing))
    return f


def as_dataset_arrays(fx=None):
    """What tests/eval_driver.py reads: frames uint8 [CLIPS, T, 3, H, W] carrying the prediction's class index as the pixel value of every
    channel, and the rest as it is."""
    fx = build() if fx is None else fx
    frames = np.ascontiguousarray(np.broadcast_to(fx["pred"][:, :, None], (CLIPS, T, 3, H, W)))
    return {"frames": frames, "target": fx["target"], "spacing": fx["spacing"], "lengths": fx["lengths"], "file_ef": fx["file_ef"]}
