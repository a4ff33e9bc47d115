"""The fixture and the CPU restatement behind tests/test_eval_report_gpu.py, checked without a GPU: the fixture holds every case the comparison
is meant to catch (tests/eval_fixture.fixture_conditions), the restatement gives the answers known by hand, its sums add over clip ranges, and
it moves when its inputs are mutated the way a wrong eval.py loop would mutate them."""
import functools

import numpy as np

from tests import eval_fixture as F
from tests import eval_reference as E

TOL = 1e-5 + 1e-9                                            # one unit of the report's rounding


def flat(rep, prefix=""):
    """{"block.key" or "block.key[i]": value} of a report."""
    out = {}
    for k, v in rep.items():
        if isinstance(v, dict):
            out.update(flat(v, f"{prefix}{k}."))
        elif isinstance(v, list):
            out.update({f"{prefix}{k}[{i}]": x for i, x in enumerate(v)})
        else:
            out[prefix + k] = v
    return out


def moved(a, b):
    """The keys of two reports of the same shape whose values differ by more than the tolerance."""
    fa, fb = flat(a), flat(b)
    assert list(fa) == list(fb)
    return [k for k in fa if abs(fa[k] - fb[k]) > TOL]


@functools.lru_cache(maxsize=None)
def whole():
    return F.report()


def test_the_fixture_holds_every_case_the_comparison_is_for():
    f = F.fixture_conditions()
    assert f["clips_the_vote_changes"] > 1
    assert f["frames_filtered"] > 0 and f["frames_not_filtered"] > 0
    assert f["pixels_filled"] > 0 and f["holes_left_above_max_area"] >= 1 and F.PARAMS["fill_max_area"] > 0
    assert f["ed_es_volumes_the_fill_moves"] >= 1
    assert f["clips_mod_batch"] != 0 and f["batches"] >= 4
    assert f["distinct_spacing_values"] == 2 * F.CLIPS and f["isotropic_spacings"] == 0
    assert f["batches_of_equal_ef"] == 0
    assert f["clips_with_ef"] >= 4 and f["distinct_pred_ef"] == f["clips_with_ef"] == f["distinct_ref_ef"] and 0.0 < abs(f["ef_pearson_r"]) < 1.0
    assert f["clips_with_one_labelled_frame"] == 1 and not f["single_frame_clip_has_ef"]
    assert f["half_clip_labelled_frames"] == F.T // 2 and f["half_clip_pred_pixels_in_unlabelled_frames"] > 0
    assert f["surface_frames_both"] > 0 and f["surface_frames_one_empty"] > 0 and f["surface_frames_unlabelled"] > 0
    assert f["clips_with_two_beats"] >= 2
    assert f["vanished_frames_after_the_chain"] > f["vote_window"] and f["vanished_clip_is_dropped"]
    assert f["short_clip_length"] < F.T and f["short_clip_systoles_with_padding"] > f["short_clip_systoles"]
    assert f["clips_it_does_not"] >= 1 and f["clips_the_target_covers"] >= 2
    assert f["file_ef_nan"] >= 1 and f["file_ef_numbers"] >= 2
    assert f["tie_distance"] > 1e-6


def test_the_other_arms_differ_and_meet_no_axis_tie_either():
    """Run C of the GPU test measures other masks (no vote, connectivity 8, every hole filled): both connectivities matter on this fixture,
    and these masks keep clear of rounding ties too."""
    fx = F.build()
    c4, c8 = (E.post_process(fx["pred"], num_classes=3, lv_class=1, vote=0, keep=k, fill=k, fill_max_area=0) for k in (4, 8))
    assert (c4["filtered"] != c8["filtered"]).any() and c4["holes"] != c8["holes"]
    assert F.tie_distance(c8["measured"], 1) > 1e-6


def test_report_has_the_documented_keys_in_order():
    rep = whole()
    ef = ["clips_with_ef", "ef_mae", "ef_bias", "ef_pearson_r", "mean_ref_ef", "mean_pred_ef"]
    assert list(rep) == ["dice_per_class", "mean_foreground_dice", "iou_per_class", "mean_foreground_iou", "lv", "lv_mm", "temporal_vote",
                         "largest_component", "fill_holes", "surface", "surface_mm", "beats"]
    assert list(rep["lv"]) == ef and list(rep["lv_mm"]) == ef + ["edv_mae_ml", "edv_bias_ml", "esv_mae_ml", "esv_bias_ml"]
    assert list(rep["temporal_vote"]) == ["radius", "frames_changed", "pixels_changed", "flips_per_frame_before", "flips_per_frame_after",
                                          "dice_per_class", "mean_foreground_dice"]
    assert list(rep["largest_component"]) == ["connectivity", "frames_changed", "pixels_removed", "dice_lv", "iou_lv"]
    assert list(rep["fill_holes"]) == ["connectivity", "max_area", "frames_changed", "holes", "pixels_filled", "dice_lv", "iou_lv"]
    assert list(rep["surface"]) == ["class", "frames", "frames_one_empty", "hd_mean", "hd95_mean", "assd_mean"]
    assert list(rep["surface_mm"]) == ["frames", "frames_one_empty", "hd_mean_mm", "hd95_mean_mm", "assd_mean_mm"]
    assert list(rep["beats"]) == ["clips", "beats_per_clip", "mean_cycle_frames", "clips_dropped_below_min", "clips_with_target", "ef_mae", "ef_bias",
                                  "ef_pearson_r", "systole_count_agreement", "vs_file_ef"]
    assert list(rep["beats"]["vs_file_ef"]) == ["clips_with_ef", "ef_mae", "ef_bias", "ef_pearson_r"]
    off = F.report(lv_class=-1, vote=0, surface_class=-1, spacing=None)
    assert list(off) == ["dice_per_class", "mean_foreground_dice", "iou_per_class", "mean_foreground_iou"]


def test_a_prediction_equal_to_the_target_scores_perfectly():
    """Without the vote (which would smooth the breathing target itself): Dice and IoU 1, every EF error 0 and r 1, every surface mean 0, the
    beats of both sides the same."""
    fx = F.build()
    rep = F.report(pred=fx["target"], vote=0)
    assert rep["dice_per_class"] == [1.0] * 3 and rep["iou_per_class"] == [1.0] * 3 and rep["mean_foreground_dice"] == 1.0
    for blk in (rep["lv"], rep["lv_mm"]):
        assert blk["clips_with_ef"] == 6 and blk["ef_mae"] == 0.0 and blk["ef_bias"] == 0.0 and blk["ef_pearson_r"] == 1.0
        assert blk["mean_ref_ef"] == blk["mean_pred_ef"] > 0.3
    assert [rep["lv_mm"][k] for k in ("edv_mae_ml", "edv_bias_ml", "esv_mae_ml", "esv_bias_ml")] == [0.0] * 4
    assert rep["largest_component"]["pixels_removed"] == 0 and rep["largest_component"]["dice_lv"] == 1.0
    assert rep["fill_holes"]["holes"] == 0 and rep["fill_holes"]["pixels_filled"] == 0 and rep["fill_holes"]["iou_lv"] == 1.0
    assert rep["surface"]["frames"] > 100 and [rep["surface"][k] for k in ("frames_one_empty", "hd_mean", "hd95_mean", "assd_mean")] == [0, 0.0, 0.0, 0.0]
    assert [rep["surface_mm"][k] for k in ("hd_mean_mm", "hd95_mean_mm", "assd_mean_mm")] == [0.0] * 3
    bt = rep["beats"]
    assert bt["clips_with_target"] == 5 and bt["ef_mae"] == 0.0 and bt["ef_pearson_r"] == 1.0 and bt["systole_count_agreement"] == 1.0
    assert bt["clips_dropped_below_min"] == 2                # the half-labelled and the single-frame clip: unlabelled frames hold no class


def test_at_one_millimetre_per_pixel_the_ml_block_repeats_the_pixel_block():
    sp = np.full((F.CLIPS, 2), 1000, np.int32)
    rep = F.report(spacing=sp, surface_class=-1, lv_beats=False)
    for k, v in rep["lv"].items():
        assert abs(rep["lv_mm"][k] - v) <= TOL, k
    # ... and a pixel^3 is a microlitre: the EDV and ESV errors in mL are those in pixel^3 / 1000
    fx = F.build()
    measured = E.post_process(fx["pred"], **{k: F.PARAMS[k] for k in ("num_classes", "lv_class", "vote", "keep", "fill", "fill_max_area")})["measured"]
    efs = [e for e in (E.clip_ef(measured[b], fx["target"][b], 1) for b in range(F.CLIPS)) if e is not None]
    for k, name in ((0, "edv"), (1, "esv")):
        err = [(p[k] - g[k]) / 1000.0 for p, g in efs]
        assert abs(rep["lv_mm"][f"{name}_mae_ml"] - sum(abs(e) for e in err) / len(err)) <= TOL and rep["lv_mm"][f"{name}_mae_ml"] > 0.01
        assert abs(rep["lv_mm"][f"{name}_bias_ml"] - sum(err) / len(err)) <= TOL


def test_the_sums_of_two_clip_ranges_add_up():
    a, b, w = flat(F.report(clip_range=(0, 3))), flat(F.report(clip_range=(3, F.CLIPS))), flat(whole())
    ints = [k for k, v in w.items() if isinstance(v, int) and k.split(".")[-1] not in ("radius", "connectivity", "max_area", "class")]
    assert len(ints) == 17, ints
    for k in ints:
        assert a[k] + b[k] == w[k], k
    assert moved(F.report(clip_range=(0, 3)), whole())       # ... and a part is not the whole


def test_the_report_moves_under_the_mutations_a_wrong_loop_would_make():
    """Each mutation is one way eval.py's loop could be wrong with numbers that stay in range; the keys it moves are printed (pytest -s)."""
    fx, ref = F.build(), whole()
    seen = {}
    # every clip measured with the spacing of the clip one batch on
    seen["spacing rows shifted by one batch"] = moved(F.report(spacing=np.roll(fx["spacing"], -F.BATCH, axis=0)), ref)
    assert {k.split(".")[0] for k in seen["spacing rows shifted by one batch"]} == {"lv_mm", "surface_mm", "beats"}
    # the unlabelled frames counted as labelled ones that hold background only
    lab = fx["target"].copy()
    lab[lab == F.IGNORE] = 0
    seen["unlabelled frames treated as labelled"] = moved(F.report(target=lab), ref)
    assert "dice_per_class[1]" in seen["unlabelled frames treated as labelled"] and "surface.frames_one_empty" in seen["unlabelled frames treated as labelled"]
    # fill, then filter, then vote, measured as it comes out
    p = dict(num_classes=3, lv_class=1, fill_max_area=F.PARAMS["fill_max_area"])
    m = E.post_process(fx["pred"], vote=0, keep=0, fill=F.PARAMS["fill"], **p)["measured"]
    m = E.post_process(m, vote=0, keep=F.PARAMS["keep"], fill=0, **p)["measured"]
    m = E.post_process(m, vote=F.PARAMS["vote"], keep=0, fill=0, **p)["measured"]
    want = F.report(surface_class=-1)
    got = F.report(pred=m, vote=0, keep=0, fill=0, surface_class=-1)
    seen["vote, filter and fill reordered"] = [k for blk in ("lv", "lv_mm", "beats") for k in moved({blk: got[blk]}, {blk: want[blk]})]
    assert any(k.startswith("lv.") for k in seen["vote, filter and fill reordered"])
    # EDV's errors reported as ESV's
    swap = {**ref, "lv_mm": {**ref["lv_mm"], **{k: ref["lv_mm"][k.replace("edv", "esv") if "edv" in k else k.replace("esv", "edv")]
                                                for k in ("edv_mae_ml", "edv_bias_ml", "esv_mae_ml", "esv_bias_ml")}}}
    seen["edv and esv swapped"] = moved(swap, ref)
    assert len(seen["edv and esv swapped"]) == 4
    # the padding frames of the short clip read as its own
    seen["lengths ignored"] = moved(F.report(lengths=np.full(F.CLIPS, F.T, np.int32)), ref)
    assert seen["lengths ignored"] and all(k.startswith("beats.") for k in seen["lengths ignored"])
    for name, keys in seen.items():
        print(f"{name}: {len(keys)} keys move: {', '.join(keys)}")
