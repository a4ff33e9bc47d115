"""eval.py's `strain` block and predict.segment_native's `strain` keys against their restatement on tests/contour_reference.py
(tests/strain_eval_fixture.py: prescribed 4-class masks, four clips of 32 x 32, one without any base interface).  tests/strain_eval_driver.py
runs eval.py in a fresh child process each time, unchanged, with the forward replaced by the prescribed prediction.  The --clip-range run is
ONE rank's sums before the all_reduce."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import contour_reference as R
from tests import strain_eval_fixture as F
from tests.test_native_eval_gpu import ROOT, differences

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(ROOT, "tests", "strain_eval_driver.py")
KEYS = ["unit", "wall_classes", "base_classes", "clips_with_strain", "gls_mae", "gls_bias", "gls_pearson_r", "mean_ref_gls", "mean_pred_gls",
        "long_axis"]


def run_eval(driver_args, overrides, tmp_path, timeout=240):
    """The JSON reports of one child process (tests/strain_eval_driver.py), one per eval.main it ran"""
    ev = subprocess.run([sys.executable, DRIVER] + driver_args + overrides + [f"run_dir={tmp_path}"], capture_output=True, text=True, timeout=timeout,
                        cwd=ROOT)
    assert ev.returncode == 0, f"strain_eval_driver exited with {ev.returncode}:\n{ev.stderr[-3000:]}"
    return [json.loads(line) for line in ev.stdout.strip().splitlines() if line.startswith("{")]


def overrides(root):
    return ["data.kind=npy_clips", f"data_path={root}", f"data.size={F.H}", f"data.frames={F.T}", f"data.num_classes={F.NCLS}",
            f"data.lv_class={F.CLS}", f"batch_size={F.BATCH}", "model.value_dim=64", "data.lv_strain=true"]


def diff(got, want):
    """test_native_eval_gpu.differences for the strain block: the unit is a string and compared as one"""
    if got.get("unit") != want["unit"]:
        return [("unit", got.get("unit"), want["unit"])]
    return differences({k: v for k, v in got.items() if k != "unit"}, {k: v for k, v in want.items() if k != "unit"})


def test_strain_block_equals_its_restatement_and_changes_no_other_key(hip, tmp_path):
    root = F.write_split(str(tmp_path / "split"))
    on, off = run_eval(["--and-without"], overrides(root), tmp_path)       # the second report: the same run with the switch off
    got, want = on["strain"], F.block(mm=True)
    print("eval.py:", got, "\nrestatement:", want)
    assert list(got) == KEYS and got["unit"] == "mm" and "lv_mm" in on
    bad = diff(got, want)
    assert not bad, f"(key, eval.py, restatement): {bad}"
    # the fixture does what it is for: every clip has a strain, the clip without an atrium has no landmarks, the cavity shortens
    assert want["clips_with_strain"] == F.CLIPS and want["long_axis"]["clips_without_landmarks"] >= 1
    assert want["long_axis"]["clips_with_landmarks"] >= 1 and want["mean_ref_gls"] < -0.05 and want["mean_pred_gls"] < -0.05
    assert "strain" not in off
    on.pop("strain")
    assert on == off


def test_one_ranks_sums_in_pixels(hip, tmp_path):
    bare = F.write_split(str(tmp_path / "bare"), spacing=False)  # no spacing: the lv block's frames, lengths in pixels
    (part,) = run_eval(["--clip-range", "1", "4"], overrides(bare), tmp_path)
    want = F.block(mm=False, clip_range=(1, 4))
    assert part["strain"]["unit"] == "px" and "lv_mm" not in part
    bad = diff(part["strain"], want)
    assert not bad, f"(key, eval.py, restatement): {bad}"
    assert want != F.block(mm=False) and want["clips_with_strain"] == 3


class _Prescribed:
    """SegmentRunner's call interface for predict.segment_native: the frames carry the class index as the byte of every plane"""
    replays = eager_calls = 0

    def __call__(self, frames, target=None):
        return torch.round(frames[:, :, 0].to(torch.float32) * 255.0).to(torch.uint8).contiguous(), None


def test_segment_native_strain_keys(hip):
    from gdkvm_amd.config import load_config
    from gdkvm_amd.predict import segment_native
    fx = F.build()
    cfg = load_config(None, [f"data.size={F.H}", f"data.num_classes={F.NCLS}", "data.lv_strain=true"])
    model = torch.nn.Linear(1, 1).cuda()                         # segment_native asks it for its device only: the runner is prescribed
    clips = [torch.from_numpy(fx["pred"][b].copy()) for b in range(F.CLIPS)]       # native size = the grid: the area average is the identity
    spacing = [tuple(float(v) for v in F.SPACING[0]), None, tuple(float(v) for v in F.SPACING[2]), tuple(float(v) for v in F.SPACING[3])]
    res = segment_native(model, cfg, clips, spacing, runner=_Prescribed())
    assert np.array_equal(res["grid_mask"].cpu().numpy(), fx["pred"])
    r5 = lambda v: round(float(v), 5)
    for b in range(F.CLIPS):
        sp = None if spacing[b] is None else F.SPACING[b]
        got = res["report"]["per_clip"][b]["strain"]
        ed, es = F.picks(fx["pred"][b], sp)
        npix, lens = F.lengths(fx["pred"][b], sp)
        _, gls, peak, led, frame, ok = R.strain_ref([l[0] for l in lens], npix, ed, es)
        _, ags, _, _, _, aok = R.strain_ref([l[2] for l in lens], npix, ed, es)
        want = {"unit": "px" if sp is None else "mm", "ok": ok, "gls": r5(gls), "peak_strain": r5(peak), "peak_frame": frame,
                "wall_ed": r5(lens[ed][0]), "wall_es": r5(lens[es][0]), "landmarks": aok, "axis_ed": r5(lens[ed][2]), "axis_es": r5(lens[es][2]),
                "axis_shortening": r5(ags)}
        assert list(got) == list(want), (b, list(got))
        for k, w in want.items():
            assert (got[k] == w) if isinstance(w, (bool, int, str)) else abs(got[k] - w) <= 1e-5 + 1e-9, (b, k, got[k], w)
        assert ok and gls < -0.05 and aok == (b != F.NO_BASE)
    plain = segment_native(model, load_config(None, [f"data.size={F.H}", f"data.num_classes={F.NCLS}"]), clips, spacing, runner=_Prescribed())
    assert all("strain" not in pc for pc in plain["report"]["per_clip"])
    for pc, qc in zip(plain["report"]["per_clip"], res["report"]["per_clip"]):
        assert {k: v for k, v in qc.items() if k != "strain"} == pc
