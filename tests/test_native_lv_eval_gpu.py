"""eval.py's native.lv block against its CPU restatement (tests/native_lv_eval_fixture.block) on the prescribed predictions of
tests/native_eval_fixture.py, written as an npy_clips tree with a spacing of the native pixel per clip, and predict.segment_native's
lv_native entry.  tests/native_eval_driver.py runs eval.py in a fresh child process each time, unchanged."""
import numpy as np
import pytest
import torch

from tests import lv_reference as LV
from tests import native_eval_fixture as F
from tests import native_lv_eval_fixture as LF
from tests import native_lv_reference as NL
from tests.test_native_eval_gpu import differences, overrides, run_eval
from tests.test_strain_eval_gpu import _Prescribed

pytestmark = pytest.mark.gpu
EF_KEYS = ["clips_with_ef", "ef_mae", "ef_bias", "ef_pearson_r", "mean_ref_ef", "mean_pred_ef"]
ML_KEYS = ["edv_mae_ml", "edv_bias_ml", "esv_mae_ml", "esv_bias_ml"]
POST = dict(vote=1, keep=4, fill=4)


def diff(got, want):
    """test_native_eval_gpu.differences for the lv block: the unit is a string and compared as one"""
    if got.get("unit") != want["unit"]:
        return [("unit", got.get("unit"), want["unit"])]
    return differences({k: v for k, v in got.items() if k != "unit"}, {k: v for k, v in want.items() if k != "unit"})


def test_native_lv_block_equals_its_restatement_and_changes_no_other_key(hip, tmp_path):
    """The post-processed mask is the one measured (the island of clip 1 would add a tenth to its volumes); the second run is the same
    report without the key."""
    root = LF.write_split(str(tmp_path / "split"))
    (with_key,) = run_eval([], overrides(root, **POST) + ["data.native_lv=true"], tmp_path)
    (without,) = run_eval([], overrides(root, **POST), tmp_path)
    got, want = with_key["native"]["lv"], LF.block(**POST)
    print("eval.py:", got, "\nrestatement:", want)
    assert list(got) == EF_KEYS + ML_KEYS + ["unit", "frames"] and got["unit"] == "mL"
    bad = diff(got, want)
    assert not bad, f"(key, eval.py, restatement): {bad}"
    assert want["clips_with_ef"] == F.CLIPS - 1 and want["frames"] == F.CLIPS * F.T and want["edv_mae_ml"] > 0
    assert diff(LF.block(), want)                             # the raw mask's block is another one
    assert "lv" not in without["native"] and list(with_key["native"])[-1] == "lv"
    with_key["native"].pop("lv")
    assert with_key == without                                # with the flag off the report is the parent's, key for key


def test_one_ranks_sums_the_raw_mask_and_the_pixel_unit(hip, tmp_path):
    root = LF.write_split(str(tmp_path / "split"))
    (part,) = run_eval(["--clip-range", "1", "4"], overrides(root) + ["data.native_lv=true", "data.native_surface_class=1"], tmp_path)
    want = LF.block(clip_range=(1, 4))
    bad = diff(part["native"]["lv"], want)
    assert not bad, f"(key, eval.py, restatement): {bad}"
    assert want != LF.block() and list(part["native"])[-2:] == ["surface", "lv"]
    bare = LF.write_split(str(tmp_path / "bare"), spacing="holes")         # one clip without a spacing: nothing is measured in mL
    (px,) = run_eval([], overrides(bare) + ["data.native_lv=true"], tmp_path)
    want = LF.block(unit="px3")
    assert list(px["native"]["lv"]) == EF_KEYS + ["unit", "frames"] and px["native"]["lv"]["unit"] == "px3"
    bad = diff(px["native"]["lv"], want)
    assert not bad, f"(key, eval.py, restatement): {bad}"


def test_native_lv_without_native_eval_is_refused(hip, tmp_path):
    root = LF.write_split(str(tmp_path / "split"))
    ev = run_eval([], [a for a in overrides(root) if a != "data.native_eval=true"] + ["data.native_lv=true"], tmp_path, check=False)
    assert ev.returncode != 0 and "data.native_lv needs data.native_eval: true and data.lv_class >= 0" in ev.stderr


def test_segment_native_lv_native_entry(hip):
    """One clip with a native spacing (rint-ed to integer um) and one without: native size = the grid, so the native masks are the
    prescribed prediction and the entry is the reference's measurement of it."""
    from gdkvm_amd.config import load_config
    from gdkvm_amd.predict import segment_native
    fx = F.build()
    base = [f"data.size={F.H}", f"data.num_classes={F.NCLS}"]
    cfg = load_config(None, base + ["data.native_eval=true", "data.native_lv=true"])
    model = torch.nn.Linear(1, 1).cuda()                         # segment_native asks it for its device only: the runner is prescribed
    clips = [torch.from_numpy(fx["pred"][b].copy()) for b in (0, 2)]
    spacing = [(308.4, 153.6), None]
    res = segment_native(model, cfg, clips, spacing, runner=_Prescribed())
    assert np.array_equal(res["grid_mask"].cpu().numpy(), fx["pred"][[0, 2]])
    assert all(np.array_equal(m.cpu().numpy(), fx["pred"][b]) for m, b in zip(res["masks"], (0, 2)))
    r5 = lambda v: round(float(v), 5)
    for k, (b, sp) in enumerate(((0, (308, 154)), (2, None))):
        pc = res["report"]["per_clip"][k]
        ms = [NL.measure(f, *(sp or (1, 1)), F.PARAMS["lv_class"]) for f in fx["pred"][b]]
        idx, val = LV.lv_ef_ref([[m["geom"][1] for m in ms]], [[m["stats"][0] for m in ms]])
        want = {"ed_frame": idx[0][0], "es_frame": idx[0][1], "valid_frames": idx[0][2], "ef": r5(val[0][2])}
        if sp is not None:
            want.update(spacing_um=list(sp), edv_ml=r5(val[0][0]), esv_ml=r5(val[0][1]))
        got = pc["lv_native"]
        assert list(got) == list(want), (k, list(got))
        for key, w in want.items():
            assert (got[key] == w) if isinstance(w, (int, list)) else abs(got[key] - w) <= 1e-5 + 1e-9, (k, key, got[key], w)
        assert got["ed_frame"] == 0 and got["es_frame"] == F.T - 1 and got["ef"] > 0.1
        assert ("lv_native_ml_omitted" in pc) == (sp is None)
    assert res["report"]["per_clip"][1]["lv_native_ml_omitted"] == "no spacing"
    plain = segment_native(model, load_config(None, base), clips, spacing, runner=_Prescribed())
    for pc, qc in zip(plain["report"]["per_clip"], res["report"]["per_clip"]):
        assert {k: v for k, v in qc.items() if not k.startswith("lv_native")} == pc
