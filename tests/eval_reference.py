"""eval.py's whole report restated on the CPU: from the predicted masks and the targets of a split to every key of the JSON line except
`split`, `clips` and `forward`, in the JSON's nesting and key order and with its round(., 5).  The masks are post-processed and measured by
the references of the single kernels (cc_reference, holes_reference, temporal_reference, lv_reference, spacing_reference, surface_reference,
beats_reference); every sum, mean, MAE, bias and Pearson r on top of them is a plain Python float or int, written out from the meaning
eval.py's docstring and the ops docstrings give each key -- clip by clip over the whole split, with no batches, no running offsets and no
flat accumulators, which are what this file is there to check.  Test infrastructure: imports nothing from the product (neither gdkvm_amd
nor eval.py) and calls none of ops.ef_summary / ef_stats / surface_summary / surface_stats / vote_summary / counts_after_largest /
class_counts_after_fill / beats_summary / beats_stats / dice_from_counts / iou_from_counts: those are the code under test."""
import math

import numpy as np

from tests import beats_reference as BT
from tests import cc_reference as C
from tests import holes_reference as HO
from tests import lv_reference as LV
from tests import spacing_reference as SP
from tests import surface_reference as SF
from tests import temporal_reference as TV

EPS = 1e-6                                                   # Dice and IoU: an absent class scores 1


def r5(v):
    """The JSON's rounding: integers as they are, floats to five decimals."""
    return v if isinstance(v, int) else round(float(v), 5)


def dice(inter, a, b):
    return (2.0 * inter + EPS) / (a + b + EPS)


def iou(inter, a, b):
    return (inter + EPS) / (a + b - inter + EPS)


def labelled_frames(target, num_classes):
    """bool [clips, T]: the frames that carry labels -- a non-empty target in some class (an IGNORE_LABEL frame has none)."""
    return (np.asarray(target) < num_classes).any((2, 3))


def post_process(pred, *, num_classes, lv_class, vote, keep, fill, fill_max_area):
    """The chain on the predicted masks of whole clips [clips, T, H, W]: the temporal vote, then the largest component of lv_class (the
    removed pixels become 0), then its holes filled.  Returns {"voted", "filtered", "filled", "measured"}: a stage that is off is None, and
    `measured` is the last stage that is on (the prediction itself when none is); `holes` counts the holes the fill found."""
    pred = np.asarray(pred)
    B, T, H, W = pred.shape
    out = {"voted": None, "filtered": None, "filled": None, "holes": 0}
    cur = pred
    if vote:
        cur = out["voted"] = TV.temporal_vote_ref(cur, num_classes, vote)[0]
    if keep and lv_class >= 0:
        cur = out["filtered"] = C.largest_component_frames(cur.reshape(B * T, H, W), lv_class, keep, 0)[0].reshape(B, T, H, W)
    if fill and lv_class >= 0:
        cur, info = HO.fill_holes_frames(cur.reshape(B * T, H, W), lv_class, fill, fill_max_area)
        cur = out["filled"] = cur.reshape(B, T, H, W)
        out["holes"] = int(info[:, 0].sum())                  # every hole of the class, filled or not
    out["measured"] = cur
    return out


def class_counts(mask, target, lab, num_classes, clips):
    """[ncls][3] Python ints = |A n B|, |A|, |B| over the labelled frames of `clips`."""
    tot = np.zeros((num_classes, 3), np.int64)
    for b in clips:
        for t in np.flatnonzero(lab[b]):
            tot += C.counts_ref(mask[b, t], target[b, t], num_classes)
    return [[int(v) for v in row] for row in tot]


def curves(clip, cls, sp=None):
    """(pixels [T], volume [T]) of one clip [T, H, W]: pixel^3 without a spacing, mL with sp = (row_um, col_um)."""
    if sp is None:
        ms = [LV.lv_measure_ref(f, cls) for f in clip]
    else:
        ms = [SP.lv_measure_mm_ref(f, int(sp[0]), int(sp[1]), cls) for f in clip]
    return [m["stats"][0] for m in ms], [m["geom"][1] for m in ms]


def compare(pairs):
    """{clips_with_ef, ef_mae, ef_bias, ef_pearson_r, mean_ref_ef, mean_pred_ef} of (predicted, reference) pairs: the error is predicted
    minus reference, r is 0 with fewer than two pairs or when either side has no variance."""
    n = len(pairs)
    if n == 0:
        return {"clips_with_ef": 0, "ef_mae": 0.0, "ef_bias": 0.0, "ef_pearson_r": 0.0, "mean_ref_ef": 0.0, "mean_pred_ef": 0.0}
    p, g = [float(a) for a, _ in pairs], [float(b) for _, b in pairs]
    mp, mg = math.fsum(p) / n, math.fsum(g) / n
    r = 0.0
    if n >= 2 and max(p) > min(p) and max(g) > min(g):
        cov = math.fsum((a - mp) * (b - mg) for a, b in zip(p, g))
        r = cov / math.sqrt(math.fsum((a - mp) ** 2 for a in p) * math.fsum((b - mg) ** 2 for b in g))
    return {"clips_with_ef": n, "ef_mae": math.fsum(abs(a - b) for a, b in zip(p, g)) / n, "ef_bias": math.fsum(a - b for a, b in zip(p, g)) / n,
            "ef_pearson_r": r, "mean_ref_ef": mg, "mean_pred_ef": mp}


def clip_ef(measured, target, cls, sp=None):
    """One clip's (predicted, target's) [EDV, ESV, EF], or None when the clip has no EF: ED and ES are the frames of the target's largest and
    smallest volume among its frames with a pixel of the class (two at least, and an EDV above 0), and the prediction is read at THOSE."""
    t_n, t_v = curves(target, cls, sp)
    p_n, p_v = curves(measured, cls, sp)
    idx, ref = LV.lv_ef_ref([t_v], [t_n])
    if idx[0][0] < 0 or not ref[0][0] > 0:
        return None
    _, got = LV.lv_ef_ref([p_v], [p_n], pick_vol=[t_v], pick_npix=[t_n])
    return got[0], ref[0]


def surface_block(pred, target, lab, cls, clips, spacing=None):
    """(frames, frames_one_empty, mean HD, mean HD95, mean ASSD) of class `cls` over the labelled frames of `clips`: the means over the frames
    where both masks have a surface (0 without one); pixels, or mm with a spacing table."""
    n = one = 0
    sums = [[], [], []]
    for b in clips:
        ts = np.flatnonzero(lab[b])
        if ts.size == 0:
            continue
        if spacing is None:
            recs = SF.surface_distance_frames(pred[b, ts], target[b, ts], cls)
            mets = [SF.metrics_ref(r) for r in recs]
        else:
            recs = SP.surface_distance_mm_frames(pred[b, ts], target[b, ts], [int(spacing[b][0]), int(spacing[b][1])], cls)
            mets = [SP.metrics_mm_ref(r) for r in recs]
        for rec, (hd, hd95, assd, valid) in zip(recs, mets):
            if valid:
                n += 1
                for s, v in zip(sums, (hd, hd95, assd)):
                    s.append(v)
            elif (int(rec[0]) > 0) != (int(rec[1]) > 0):
                one += 1
    return (n, one) + tuple(math.fsum(s) / n if n else 0.0 for s in sums)


def eval_report_ref(pred, target, *, num_classes, lv_class, keep, fill, fill_max_area, vote, surface_class, spacing, lengths, lv_beats,
                    beat_distance, beat_permille, file_ef, clip_range=None):
    """pred, target uint8 [clips, T, H, W] (255 = IGNORE_LABEL); keep, fill = 0, 4 or 8; vote = 0 or the radius; surface_class = -1 or a class;
    spacing = None or [clips][2] = (row_um, col_um); lengths [clips] = every clip's own frames; file_ef = None or [clips] per cent with NaN
    where a file has none; clip_range = (lo, hi) restricts every sum to those clips.  Returns eval.py's report without split, clips and
    forward."""
    pred, target = np.asarray(pred), np.asarray(target)
    assert pred.dtype == np.uint8 and target.dtype == np.uint8 and pred.shape == target.shape and pred.ndim == 4
    if clip_range is not None:                               # the clips of the range are a split of their own: nothing reaches across clips
        part = lambda a: None if a is None else a[clip_range[0]:clip_range[1]]
        pred, target, spacing, lengths, file_ef = (part(a) for a in (pred, target, spacing, lengths, file_ef))
    B, T, H, W = pred.shape
    clips = range(B)
    lab = labelled_frames(target, num_classes)
    lv_on = lv_class >= 0
    stages = post_process(pred, num_classes=num_classes, lv_class=lv_class, vote=vote, keep=keep, fill=fill, fill_max_area=fill_max_area)
    voted, filtered, filled, measured = (stages[k] for k in ("voted", "filtered", "filled", "measured"))

    def dice_keys(counts, with_iou):
        d, j = [dice(*c) for c in counts], [iou(*c) for c in counts]
        fg = max(len(counts) - 1, 1)
        keys = {"dice_per_class": [r5(v) for v in d], "mean_foreground_dice": r5(sum(d[1:]) / fg)}
        if with_iou:
            keys.update({"iou_per_class": [r5(v) for v in j], "mean_foreground_iou": r5(sum(j[1:]) / fg)})
        return keys

    # Dice and IoU of the UNFILTERED prediction over the labelled frames
    res = dice_keys(class_counts(pred, target, lab, num_classes, clips), True)

    if lv_on:
        # one EF per clip from the measured mask, against the target's, in pixel^3 ...
        efs = [e for e in (clip_ef(measured[b], target[b], lv_class) for b in clips) if e is not None]
        res["lv"] = {k: r5(v) for k, v in compare([(p[2], g[2]) for p, g in efs]).items()}
        if spacing is not None:
            # ... and in mL with every clip's own spacing: ED and ES are picked on the target's mL curve
            mls = [e for e in (clip_ef(measured[b], target[b], lv_class, spacing[b]) for b in clips) if e is not None]
            blk = compare([(p[2], g[2]) for p, g in mls])
            for name, k in (("edv", 0), ("esv", 1)):
                err = [p[k] - g[k] for p, g in mls]
                blk[f"{name}_mae_ml"] = math.fsum(abs(e) for e in err) / max(len(err), 1)
                blk[f"{name}_bias_ml"] = math.fsum(err) / max(len(err), 1)
            res["lv_mm"] = {k: r5(v) for k, v in blk.items()}

    if vote:
        # changes and flips over ALL frames of the clips, the voted mask's Dice over the labelled ones
        changed = [int((voted[b, t] != pred[b, t]).sum()) for b in clips for t in range(T)]
        before = sum(int((pred[b, t] != pred[b, t - 1]).sum()) for b in clips for t in range(1, T))
        after = sum(int((voted[b, t] != voted[b, t - 1]).sum()) for b in clips for t in range(1, T))
        nfr = max(len(changed), 1)
        res["temporal_vote"] = {"radius": vote, "frames_changed": sum(1 for c in changed if c > 0), "pixels_changed": sum(changed),
                                "flips_per_frame_before": r5(before / nfr), "flips_per_frame_after": r5(after / nfr),
                                **dice_keys(class_counts(voted, target, lab, num_classes, clips), False)}

    if keep and lv_on:
        # what the filter removed from the (voted) mask over ALL frames, the filtered mask's Dice / IoU of the class over the labelled ones
        src = voted if vote else pred
        removed = [int(((src[b, t] == lv_class) & (filtered[b, t] != lv_class)).sum()) for b in clips for t in range(T)]
        c = class_counts(filtered, target, lab, num_classes, clips)[lv_class]
        res["largest_component"] = {"connectivity": keep, "frames_changed": sum(1 for v in removed if v > 0), "pixels_removed": sum(removed),
                                    "dice_lv": r5(dice(*c)), "iou_lv": r5(iou(*c))}

    if fill and lv_on:
        # the holes of the class in the mask the fill received and what it filled over ALL frames, the filled mask's Dice / IoU of the class
        src = filtered if keep else voted if vote else pred
        added = [int(((filled[b, t] == lv_class) & (src[b, t] != lv_class)).sum()) for b in clips for t in range(T)]
        c = class_counts(filled, target, lab, num_classes, clips)[lv_class]
        res["fill_holes"] = {"connectivity": fill, "max_area": fill_max_area, "frames_changed": sum(1 for v in added if v > 0), "holes": stages["holes"],
                             "pixels_filled": sum(added), "dice_lv": r5(dice(*c)), "iou_lv": r5(iou(*c))}

    if surface_class >= 0:
        # the surface distances of the UNFILTERED prediction
        n, one, hd, hd95, assd = surface_block(pred, target, lab, surface_class, clips)
        res["surface"] = {"class": surface_class, "frames": n, "frames_one_empty": one, "hd_mean": r5(hd), "hd95_mean": r5(hd95), "assd_mean": r5(assd)}
        if spacing is not None:
            n, one, hd, hd95, assd = surface_block(pred, target, lab, surface_class, clips, spacing)
            res["surface_mm"] = {"frames": n, "frames_one_empty": one, "hd_mean_mm": r5(hd), "hd95_mean_mm": r5(hd95), "assd_mean_mm": r5(assd)}

    if lv_beats and lv_on:
        # beat by beat on the measured mask's curves over every clip's OWN frames; the target is a reference only where it labels all of them
        args = dict(distance=beat_distance, permille=beat_permille)
        n_kept = n_beats = n_cyc = dropped = with_target = agree = 0
        cycles, vs_target, vs_file = [], [], []
        for b in clips:
            sp = None if spacing is None else spacing[b]
            ln = min(max(int(lengths[b]), 0), T)
            area, vol = curves(measured[b], lv_class, sp)
            _, _, (info,), (summ,) = BT.lv_beats_ref([area], [vol], [ln], **args)
            nb, systoles, below, _ = info
            if below > 0:                                     # the class vanished in a frame: a false systole, the clip is dropped
                dropped += 1
            else:
                n_kept += 1
                n_beats += nb
                if systoles >= 2:
                    n_cyc += 1
                    cycles.append(summ[3])
                f = float("nan") if file_ef is None else float(file_ef[b])
                if nb >= 1 and not math.isnan(f):
                    vs_file.append((summ[0], f / 100.0))
            if bool(lab[b, :ln].all()):
                with_target += 1
                t_area, t_vol = curves(target[b], lv_class, sp)
                _, _, (t_info,), (t_summ,) = BT.lv_beats_ref([t_area], [t_vol], [ln], **args)
                agree += int(t_info[1] == systoles)
                if nb >= 1 and below == 0 and t_info[0] >= 1 and t_info[2] == 0:
                    vs_target.append((summ[0], t_summ[0]))
        st = compare(vs_target)
        res["beats"] = {"clips": B, "beats_per_clip": r5(n_beats / max(n_kept, 1)), "mean_cycle_frames": r5(math.fsum(cycles) / max(n_cyc, 1)),
                        "clips_dropped_below_min": dropped, "clips_with_target": with_target, "ef_mae": r5(st["ef_mae"]), "ef_bias": r5(st["ef_bias"]),
                        "ef_pearson_r": r5(st["ef_pearson_r"]), "systole_count_agreement": r5(agree / with_target if with_target else 0.0)}
        if file_ef is not None:
            st = compare(vs_file)
            res["beats"]["vs_file_ef"] = {k: r5(st[k]) for k in ("clips_with_ef", "ef_mae", "ef_bias", "ef_pearson_r")}
    return res
