"""eval.py's `native` block against its CPU restatement (tests/native_reference.native_block) on prescribed predictions of an npy_clips tree
whose clips have native targets of distinct sizes (tests/native_eval_fixture.py), and every other key against the same run's report without
data.native_eval.  tests/native_eval_driver.py runs eval.py in a fresh child process each time.  The --clip-range run is ONE rank's sums
before the all_reduce; the sum of the ranks' integers itself needs a job of two ranks."""
import json
import os
import subprocess
import sys

import pytest

from tests import native_eval_fixture as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "native_eval_driver.py")
# Both sides print rounded to 1e-5, and the values behind them come from the same integers: they differ by at most one unit of the print.
TOL = 1e-5 + 1e-9


def run_eval(driver_args, overrides, tmp_path, timeout=240, check=True):
    ev = subprocess.run([sys.executable, DRIVER] + driver_args + overrides + [f"run_dir={tmp_path}"], capture_output=True, text=True, timeout=timeout,
                        cwd=ROOT)
    if not check:
        return ev
    assert ev.returncode == 0, f"native_eval_driver exited with {ev.returncode}:\n{ev.stderr[-3000:]}"
    return [json.loads(line) for line in ev.stdout.strip().splitlines() if line.startswith("{")]


def differences(got, want, where=""):
    """[(key, eval.py's, the restatement's)] where two blocks differ: other key lists, integers that are not equal, floats (and lists of
    them) further apart than TOL -- through every nested block."""
    if list(got) != list(want):
        return [(where + "keys", list(got), list(want))]
    bad = []
    for k in want:
        g, w = got[k], want[k]
        if isinstance(w, dict):
            bad += differences(g, w, f"{where}{k}.") if isinstance(g, dict) else [(where + k, g, w)]
        elif isinstance(w, list):
            if not (isinstance(g, list) and len(g) == len(w) and all(abs(a - b) <= TOL for a, b in zip(g, w))):
                bad.append((where + k, g, w))
        elif isinstance(g, int) or isinstance(w, int):
            if not (isinstance(g, int) and isinstance(w, int) and g == w):
                bad.append((where + k, g, w))
        elif not abs(g - w) <= TOL:
            bad.append((where + k, g, w))
    return bad


def overrides(root, vote=0, keep=0, fill=0):
    return ["data.kind=npy_clips", f"data_path={root}", f"data.size={F.H}", f"data.frames={F.T}", f"data.num_classes={F.NCLS}",
            f"data.lv_class={F.PARAMS['lv_class']}", f"data.temporal_vote={vote}", f"data.lv_keep_largest={keep}", f"data.lv_fill_holes={fill}",
            f"batch_size={F.BATCH}", "model.value_dim=64", "data.native_eval=true"]


@pytest.mark.parametrize("post", [dict(), dict(vote=1, keep=4, fill=4)], ids=["raw", "post"])
def test_native_block_equals_its_restatement(hip, tmp_path, post):
    """5 clips of 5 native sizes in batches of 2 (the last batch short), one clip labelled in one frame only.  The second report is the same
    run without data.native_eval: every other key must be equal."""
    root = F.write_split(str(tmp_path / "split"))
    on, off = run_eval(["--and-without"], overrides(root, **post), tmp_path)
    assert list(on)[-1] == "native" and "native" not in off
    want = F.block(**post)
    print("eval.py:", on["native"], "\nrestatement:", want)
    bad = differences(on["native"], want)
    assert not bad, f"(key, eval.py, restatement): {bad}"
    assert {k: v for k, v in on.items() if k != "native"} == off
    assert want["frames"] == F.CLIPS * F.T - 2
    assert want["pixels"] == sum((1 if b == F.HALF_LABELLED else F.T) * h0 * w0 for b, (h0, w0) in enumerate(F.SIZES))
    assert ("post" in want) == bool(post)
    if post:                                                  # the clean-ups removed the island: the post block is another one
        assert want["post"]["dice_per_class"] != {k: v for k, v in want.items() if k != "post"}["dice_per_class"]


def test_one_ranks_sums_are_its_own_clips(hip, tmp_path):
    """The clips 1 .. 3 only, as one of several ranks would measure them: i starts at the shard's first clip, for the targets and the sizes."""
    root = F.write_split(str(tmp_path / "split"))
    (on,) = run_eval(["--clip-range", "1", "4"], overrides(root), tmp_path)
    want = F.block(clip_range=(1, 4))
    bad = differences(on["native"], want)
    assert not bad, f"(key, eval.py, restatement): {bad}"
    assert want != F.block()


def test_a_clip_without_a_native_target_is_named(hip, tmp_path):
    root = F.write_split(str(tmp_path / "split"), native="holes")
    ev = run_eval([], overrides(root), tmp_path, check=False)
    assert ev.returncode != 0 and "data.native_eval needs a dataset with a native target for every clip" in ev.stderr
