"""eval.py's `biplane` block against its CPU restatement (tests/biplane_reference.biplane_block_ref) on prescribed predictions of a split of
patients' views (tests/biplane_eval_fixture.py), and every other key against the same run's report without data.lv_biplane.
tests/biplane_eval_driver.py runs eval.py in a fresh child process each time.  What one process cannot show is the sum of the ranks' tables:
the --clip-range run below is ONE rank's view before that sum (the pairs it measured whole are reported, the pair its range splits has no
target), checked against the restatement of exactly that; the all_reduce itself needs a job of two ranks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import biplane_eval_fixture as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "biplane_eval_driver.py")
# Both sides print rounded to 1e-5, and the values behind them agree to about 1e-12: they differ by at most one unit of the print.
TOL = 1e-5 + 1e-9


def run_eval(driver_args, overrides, tmp_path, timeout=240, check=True):
    ev = subprocess.run([sys.executable, DRIVER] + driver_args + overrides + [f"run_dir={tmp_path}"], capture_output=True, text=True, timeout=timeout,
                        cwd=ROOT)
    if not check:
        return ev
    assert ev.returncode == 0, f"biplane_eval_driver exited with {ev.returncode}:\n{ev.stderr[-3000:]}"
    return [json.loads(line) for line in ev.stdout.strip().splitlines() if line.startswith("{")], ev.stderr


def differences(got, want, where=""):
    """[(key, eval.py's, the restatement's)] where two blocks differ: other key lists, integers that are not equal, floats further apart than
    TOL -- through every nested block."""
    if list(got) != list(want):
        return [(where + "keys", list(got), list(want))]
    bad = []
    for k in want:
        g, w = got[k], want[k]
        if isinstance(w, dict):
            bad += differences(g, w, f"{where}{k}.") if isinstance(g, dict) else [(where + k, g, w)]
        elif isinstance(g, int) or isinstance(w, int):
            if not (isinstance(g, int) and isinstance(w, int) and g == w):
                bad.append((where + k, g, w))
        elif not abs(g - w) <= TOL:
            bad.append((where + k, g, w))
    return bad


def split_file(tmp, spacing=True):
    path = os.path.join(tmp, "patients.npz" if spacing else "patients_no_spacing.npz")
    np.savez(path, **F.as_dataset_arrays(spacing))
    return path


def overrides(keep=0, lv_class=1):
    return ["data.size=64", f"data.frames={F.T}", f"data.num_classes={F.PARAMS['num_classes']}", f"data.lv_class={lv_class}",
            f"data.lv_keep_largest={keep}", f"batch_size={F.BATCH}", "model.value_dim=64", "data.lv_biplane=true"]


@pytest.mark.parametrize("keep", [0, 4])
def test_biplane_block_equals_its_restatement(hip, tmp_path, keep):
    """7 clips in batches of 2: every pair straddles two batches.  keep = 0: everything else off; keep = 4: the islands of clips 2 and 5 are
    removed before the measurement.  The second report is the same run without data.lv_biplane: every other key must be equal."""
    (on, off), err = run_eval(["--prescribed", split_file(str(tmp_path)), "--and-without"], overrides(keep), tmp_path)
    assert list(on)[-1] == "biplane" and "biplane" not in off
    want = F.block(keep=keep)
    print("eval.py:", on["biplane"], "\nrestatement:", want)
    bad = differences(on["biplane"], want)
    assert not bad, f"(key, eval.py, restatement): {bad}"
    assert {k: v for k, v in on.items() if k != "biplane"} == off
    assert want["pairs"] == 3 and want["patients_single_view"] == 1 and want["pairs_with_target"] == 2 and want["vs_file"]["pairs_with_ef"] == 2
    assert "ef_percent of clips 1 (2CH) and 2 (4CH) differ" in err and "edv_ml of clips 1 (2CH) and 2 (4CH) differ" in err


def test_one_ranks_tables_hold_its_own_pairs(hip, tmp_path):
    """The clips 0 .. 3 only, as the first of two ranks would measure them: pair (1, 2) is whole, pair (3, 4) is split by the range and pair
    (5, 6) is the other rank's -- before the ranks' tables are added the block reports the whole split's pair table and one pair with a target."""
    (on,), _ = run_eval(["--prescribed", split_file(str(tmp_path)), "--clip-range", "0", "4"], overrides(0), tmp_path)
    want = F.block(clip_range=(0, 4))
    bad = differences(on["biplane"], want)
    assert not bad, f"(key, eval.py, restatement): {bad}"
    assert want["pairs"] == 3 and want["pairs_with_target"] == 1 and want["vs_file"]["pairs_with_ef"] == 1


def test_what_is_missing_is_named(hip, tmp_path):
    ev = run_eval(["--prescribed", split_file(str(tmp_path), spacing=False)], overrides(0, lv_class=-1), tmp_path, check=False)
    assert ev.returncode != 0 and "data.lv_biplane needs data.lv_class >= 0 and a pixel spacing for every clip" in ev.stderr
    assert "patient and view" not in ev.stderr
