"""eval.py's whole report against its CPU restatement (tests/eval_reference.py): every key of the JSON line, on prescribed predictions that
hold something to vote, filter, fill, drop and leave out (tests/eval_fixture.py; tests/test_eval_report_cpu.py asserts that they do), and on
the recorded masks of the real forward.  tests/eval_driver.py runs eval.py in a fresh child process each time."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import eval_fixture as F
from tests import eval_reference as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "eval_driver.py")
# Both sides print rounded to 1e-5, and away from axis ties the values behind them agree to about 1e-12 (test_lv_measure_gpu.py,
# test_spacing_gpu.py): they differ by at most one unit of the print.
TOL = 1e-5 + 1e-9


def run_eval(driver_args, overrides, tmp_path, timeout=240):
    ev = subprocess.run([sys.executable, DRIVER] + driver_args + overrides + [f"run_dir={tmp_path}"], capture_output=True, text=True, timeout=timeout,
                        cwd=ROOT)
    assert ev.returncode == 0, f"eval_driver exited with {ev.returncode}:\n{ev.stderr[-3000:]}"
    return json.loads(ev.stdout.strip().splitlines()[-1])


def differences(got, want, where=""):
    """[(key, eval.py's, the restatement's)] where two reports differ: other key lists, integers that are not equal, floats further apart than
    TOL -- through every nested block and list."""
    if list(got) != list(want):
        return [(where + "keys", list(got), list(want))]
    bad = []
    for k in want:
        g, w = got[k], want[k]
        if isinstance(w, dict):
            bad += differences(g, w, f"{where}{k}.") if isinstance(g, dict) else [(where + k, g, w)]
            continue
        gs, ws = (g, w) if isinstance(w, list) else ([g], [w])
        if not isinstance(gs, list) or len(gs) != len(ws):
            bad.append((where + k, g, w))
            continue
        for n, (a, b) in enumerate(zip(gs, ws)):
            if isinstance(a, int) or isinstance(b, int):
                ok = isinstance(a, int) and isinstance(b, int) and a == b
            else:
                ok = abs(a - b) <= TOL
            if not ok:
                bad.append((f"{where}{k}[{n}]" if isinstance(w, list) else where + k, a, b))
    return bad


def assert_reports_equal(got, want):
    bad = differences(got, want)
    assert not bad, f"(key, eval.py, restatement): {bad}"


def product_part(rep, clips):
    assert rep["split"] == "val" and rep["clips"] == clips and list(rep)[:3] == ["split", "clips", "forward"]
    return {k: v for k, v in rep.items() if k not in ("split", "clips", "forward")}


def split_file(tmp, spacing=True):
    arrays = F.as_dataset_arrays()
    if not spacing:
        del arrays["spacing"]
    path = os.path.join(tmp, "split.npz" if spacing else "split_no_spacing.npz")
    np.savez(path, **arrays)
    return path


def overrides(p, precision="bf16"):
    return ["data.size=64", f"data.frames={F.T}", f"data.num_classes={p['num_classes']}", f"data.lv_class={p['lv_class']}",
            f"data.temporal_vote={p['vote']}", f"data.lv_keep_largest={p['keep']}", f"data.lv_fill_holes={p['fill']}",
            f"data.lv_fill_max_area={p['fill_max_area']}", f"data.surface_class={p['surface_class']}", "data.lv_beats=true",
            f"data.beat_distance={p['beat_distance']}", f"batch_size={F.BATCH}", "model.value_dim=64", f"precision={precision}"]


def test_eval_report_equals_its_restatement_with_everything_on(hip, tmp_path):
    """Run A: vote 1, largest 4-connected component, holes of up to 6 pixels filled, surface class 2, beats, per-clip spacings, lengths and
    file EFs; 7 clips in batches of 2 (three captured-shape batches and a short one, collected one batch behind their submission)."""
    got = run_eval(["--prescribed", split_file(str(tmp_path))], overrides(F.PARAMS), tmp_path)
    assert_reports_equal(product_part(got, F.CLIPS), F.report())


def test_eval_report_of_a_later_shard_equals_its_restatement(hip, tmp_path):
    """Run B: the clips 3 .. 6 only, as a second rank would see them: the shard starts at an odd clip in the middle of run A's second batch,
    so every row of the spacing, length and file-EF tables must be found from lo on."""
    lo, hi = 3, F.CLIPS
    got = run_eval(["--prescribed", split_file(str(tmp_path)), "--clip-range", str(lo), str(hi)], overrides(F.PARAMS), tmp_path)
    assert_reports_equal(product_part(got, F.CLIPS), F.report(clip_range=(lo, hi)))


def test_eval_report_equals_its_restatement_on_the_other_arms(hip, tmp_path):
    """Run C: connectivity 8 for both filters, holes of any size, no vote, no spacing (no _mm blocks; the beats run on pixel^3 volumes),
    fp32 frames, surface class 1."""
    p = {**F.PARAMS, "keep": 8, "fill": 8, "fill_max_area": 0, "vote": 0, "surface_class": 1}
    got = run_eval(["--prescribed", split_file(str(tmp_path), spacing=False)], overrides(p, precision="fp32"), tmp_path)
    want = F.report(spacing=None, **{k: p[k] for k in ("keep", "fill", "fill_max_area", "vote", "surface_class")})
    assert "lv_mm" not in want and "surface_mm" not in want and "temporal_vote" not in want and want["fill_holes"]["max_area"] == 0
    assert_reports_equal(product_part(got, F.CLIPS), want)


RECORDED_SEED = 0


def test_eval_report_equals_its_restatement_on_the_recorded_real_forward(hip, tmp_path):
    """The real SegmentRunner (graph replays, two forwards in flight) on the synthetic validation split of 32 clips of 4 frames of 64 x 64 in
    batches of 4, seeded random weights, with the vote, both filters and the surface distances on: the masks of every get() are recorded, and
    the report must be the restatement's of those masks and the dataset's targets.  Fails, not skips, if the recorded masks of all batches
    are equal or hold no pixel of class 1.  seed=0, chosen on the first run on an MI355X: the recorded masks hold 173891 pixels of class 0 and
    350397 of class 1 (none of 2 and 3) and no two batches are equal; each of the seeds 1 .. 5 puts one class on every pixel."""
    from gdkvm_amd.data import SyntheticEchoClips
    p = dict(num_classes=4, lv_class=1, vote=1, keep=4, fill=4, fill_max_area=0, surface_class=1)
    rec = str(tmp_path / "masks.npz")
    got = run_eval(["--record", rec],
                   ["data.size=64", "data.frames=4", "batch_size=4", "model.value_dim=64", f"seed={RECORDED_SEED}", f"data.temporal_vote={p['vote']}",
                    f"data.lv_keep_largest={p['keep']}", f"data.lv_fill_holes={p['fill']}", f"data.surface_class={p['surface_class']}"], tmp_path)
    with np.load(rec) as z:
        masks, batches = z["masks"], z["batches"].tolist()
    ds = SyntheticEchoClips(32, 4, 64, num_classes=4, seed=RECORDED_SEED + 7919, as_uint8=True)
    target = np.stack([ds[i][1].numpy() for i in range(len(ds))])
    assert masks.shape == target.shape == (32, 4, 64, 64) and masks.dtype == np.uint8 and batches == [4] * 8
    assert got["forward"]["graph_replays"] >= 6 and got["forward"]["graph_replays"] + got["forward"]["eager_calls"] == 8
    pixels = [int((masks == c).sum()) for c in range(4)]
    print("recorded masks: pixels per class", pixels, "distinct batches", len({masks[k:k + 4].tobytes() for k in range(0, 32, 4)}))
    assert pixels[1] > 0, pixels
    assert len({masks[k:k + 4].tobytes() for k in range(0, 32, 4)}) > 1
    want = E.eval_report_ref(masks, target, spacing=None, lengths=[4] * 32, lv_beats=False, beat_distance=20, beat_permille=500, file_ef=None, **p)
    assert_reports_equal(product_part(got, 32), want)
