"""eval.py's native.surface block against its CPU restatement (tests/native_surface_eval_fixture.block) on the prescribed predictions of
tests/native_eval_fixture.py, written as an npy_clips tree with a spacing of the native pixel per clip.  tests/native_eval_driver.py runs
eval.py in a fresh child process each time, unchanged.  The --clip-range run is ONE rank's sums before the all_reduce."""
import pytest

from tests import native_eval_fixture as F
from tests import native_surface_eval_fixture as SF
from tests.test_native_eval_gpu import differences, overrides, run_eval

pytestmark = pytest.mark.gpu
KEYS = ["class", "unit", "frames", "frames_one_empty", "hd_mean", "hd95_mean", "assd_mean"]


def diff(got, want):
    """test_native_eval_gpu.differences for the surface block: the unit is a string and compared as one"""
    if got.get("unit") != want["unit"]:
        return [("unit", got.get("unit"), want["unit"])]
    return differences({k: v for k, v in got.items() if k != "unit"}, {k: v for k, v in want.items() if k != "unit"})


def on(root):
    return overrides(root) + [f"data.native_surface_class={SF.CLS}"]


def test_native_surface_block_equals_its_restatement_and_changes_no_other_key(hip, tmp_path):
    root = SF.write_split(str(tmp_path / "split"))
    (with_key,) = run_eval([], on(root), tmp_path)
    (without,) = run_eval([], overrides(root), tmp_path)
    got, want = with_key["native"]["surface"], SF.block()
    print("eval.py:", got, "\nrestatement:", want)
    assert list(got) == KEYS and got["unit"] == "mm"
    bad = diff(got, want)
    assert not bad, f"(key, eval.py, restatement): {bad}"
    assert want["frames"] == F.CLIPS * F.T - 2 and want["hd_mean"] > 0 and want["assd_mean"] > 0
    assert "surface" not in without["native"]                 # the second run: the same report without the block
    with_key["native"].pop("surface")
    assert with_key == without


def test_one_ranks_sums_and_the_pixel_unit(hip, tmp_path):
    root = SF.write_split(str(tmp_path / "split"))
    (part,) = run_eval(["--clip-range", "1", "4"], on(root), tmp_path)
    want = SF.block(clip_range=(1, 4))
    bad = diff(part["native"]["surface"], want)
    assert not bad, f"(key, eval.py, restatement): {bad}"
    assert want != SF.block()
    bare = SF.write_split(str(tmp_path / "bare"), spacing="holes")         # one clip without a spacing: nothing is measured in mm
    (px,) = run_eval([], on(bare), tmp_path)
    want = SF.block(unit="px")
    assert px["native"]["surface"]["unit"] == "px"
    bad = diff(px["native"]["surface"], want)
    assert not bad, f"(key, eval.py, restatement): {bad}"


def test_native_surface_class_without_native_eval_is_refused(hip, tmp_path):
    root = SF.write_split(str(tmp_path / "split"))
    ev = run_eval([], [a for a in on(root) if a != "data.native_eval=true"], tmp_path, check=False)
    assert ev.returncode != 0 and "data.native_surface_class = 1 needs data.native_eval: true" in ev.stderr
