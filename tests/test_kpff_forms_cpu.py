"""tests/kpff_forms.py against csrc/kpff.hip, and the cases of tests/test_kpff_train_forms_gpu.py against tests/kpff_forms.py: (a) every
constant equals the one in the .hip file and every restated expression still stands there, so an edited tile size, threshold or grid fails
here until the helper follows; (b) on 256 compute units and on the entry point's fallback (257 tiles), each GPU case selects the form,
the tile shapes and the trip counts it is there for; (c) the bf16 kernel's float-reciprocal divisions are exact for those cases."""
import os
import re

import numpy as np
import pytest

from tests import grid_caps as gc
from tests import kpff_forms as kf

CU_COUNTS = (256, kf.SINGLE_BELOW_FALLBACK - kf.SINGLE_BELOW_OVER_CUS)      # an MI355X, and what the entry point assumes without a count


@pytest.mark.parametrize("name", sorted(kf.CONSTANTS))
def test_constant_equals_the_source(name):
    assert kf.source_constant(name) == kf.CONSTANTS[name][0] == getattr(kf, name)


@pytest.mark.parametrize("name", sorted(kf.CONSTANTS))
def test_a_changed_constant_is_noticed(name, tmp_path):
    """The reader reads the number itself: from a copy of the source with the literals of this constant raised by one it returns another value."""
    value, fname, where, rx = kf.CONSTANTS[name]
    with open(os.path.join(gc.CSRC, fname)) as f:
        text = f.read()
    scope = text if where is None else gc.function_body(text, where)
    m = re.search(rx, scope)
    bumped = re.sub(r"\d+", lambda d: str(int(d.group()) + 1), m.group(1))
    edited = scope[:m.start(1)] + bumped + scope[m.end(1):]
    assert text.count(scope) == 1
    (tmp_path / fname).write_text(text.replace(scope, edited))
    assert kf.source_constant(name, str(tmp_path)) != value


@pytest.mark.parametrize("line", kf.SOURCE_LINES)
def test_restated_expression_stands_in_the_source(line):
    with open(os.path.join(gc.CSRC, "kpff.hip")) as f:
        assert line in f.read()


def test_the_limits_are_the_same_160_kib():
    assert kf.LDS_LIMIT == kf.LDS_LIMIT_TILE == kf.LDS_LIMIT_PAIR == kf.LDS_LIMIT_SPLIT == kf.LDS_LIMIT_EXACT == 163840
    assert kf.PACKED_SB == kf.PACKED_TOKENS and kf.PACKED_LDS_ROWS == 2 * kf.PACKED_SB


# ------------------------------------------------------------------------------------------------------------------ (b)
def test_training_configurations_take_the_large_forms():
    """configs[1] (512 frames of 7 x 7) and configs[2] (160 frames of 16 x 16) at the default widths: what the GPU cases stand in for."""
    t = kf.tiling(7, 7)
    assert t.tiles == 1 and kf.bf16_form(512 * t.tiles, 256, t.rows * t.cols, 576).form == "packed56"
    t = kf.tiling(16, 16)
    assert t.tiles == 4 and kf.bf16_form(160 * t.tiles, 256, t.rows * t.cols, 576).form == "pair"
    assert kf.bwd_pre_trips(512 * 49, 256).trips == 13


def test_tile_shapes_of_the_cases():
    shape = {k: kf.tiling(*v[0]) for k, v in kf.CASES.items()}
    assert [shape[k].tiles for k in "abcdefgh"] == [1, 1, 4, 2, 4, 4, 2, 1]
    assert shape["a"].tokens == [49] and shape["h"].tokens == [15]
    assert shape["c"].rows == 4 and shape["c"].tokens == [56, 56, 56, 28]                     # a ragged last band
    assert shape["d"].bands == [(8, 7), (6, 7)]
    assert shape["e"].tokens == [64] * 4 and shape["e"].full_w
    assert not shape["f"].full_w and shape["f"].bands == [(4, 16), (4, 3), (2, 16), (2, 3)]   # column blocks of 16 and 3, a ragged band
    assert shape["g"].bands == [(12, 5), (9, 5)] and shape["g"].tokens[0] == 60 > kf.PACKED_TOKENS
    assert all(shape[k].full_w for k in "abcdegh")
    assert kf.tiling(1, 1).tokens == [1] and not kf.tiling(8, 32).full_w and kf.tiling(32, 32).tiles == 16


@pytest.mark.parametrize("cus", CU_COUNTS)
@pytest.mark.parametrize("case", sorted(kf.CASES))
def test_each_case_selects_its_form_at_the_threshold(case, cus):
    (h, w), (ck, cv, cp), form, odd = kf.CASES[case]
    t = kf.tiling(h, w)
    assert kf.arm("bf16", ck, cv, cp) == "bf16" and kf.arm("fp32", ck, cv, cp) == "split" and kf.arm("fp32", ck, cv, cp, workspace=False) == "exact"
    bt = kf.threshold_bt(h, w, cus, odd)
    total, cin = bt * t.tiles, cp + ck + cv
    f = kf.bf16_form(total, cus, t.rows * t.cols, cin)
    assert f.form == form and total >= cus + 1 and f.blocks == (total + 1) // 2 and f.threads == 512 and f.lds <= kf.LDS_LIMIT
    assert f.idle_second == bool(total % 2) and (total % 2 == 1 or not odd)           # an invalid second sub-tile in the last workgroup
    assert (bt - 1) * t.tiles < cus + 1 or (odd and (bt - 2) * t.tiles < cus + 1)     # ... and no more frames than that takes
    # one frame fewer than the threshold, the small batch of the save tests and every slice of the bit comparison: the single-tile form
    assert kf.bf16_form(cus, cus, t.rows * t.cols, cin).form == "single"
    assert kf.bf16_form(kf.SMALL_BT * t.tiles, cus, t.rows * t.cols, cin).form == "single"
    sl = kf.slices(bt, h, w, cus)
    assert sl[0][0] == 0 and sl[-1][1] == bt and all(a[1] == b[0] for a, b in zip(sl, sl[1:])) and len(sl) >= 2
    assert sl[0][1] % 2 == 1                                           # the first cut is at an odd frame
    for f0, f1 in sl:
        g = kf.bf16_form((f1 - f0) * t.tiles, cus, t.rows * t.cols, cin)
        assert f1 > f0 and g.form == "single" and g.threads == 256 and g.blocks == (f1 - f0) * t.tiles
    if t.tiles == 1:
        assert (sl[0][1] * t.tiles) % 2 == 1                           # a slice starts on the second sub-tile of a workgroup's pair
    if case == "a":
        assert cp < f.ob_step == 128                                   # waves 4 .. 7 have no output tile
    if case == "b":
        assert cp == 2 * f.ob_step and cin == 576                      # two rounds per wave at the default widths
    assert f.sb == (56 if form == "packed56" else 64) and max(t.tokens) <= f.sb


def test_arms_of_the_save_cases():
    for h, w, ck, cv, cp in kf.SAVES_EXACT:
        assert kf.arm("bf16", ck, cv, cp) == "exact" and kf.arm("fp32", ck, cv, cp) == "exact" and kf.arm("fp32", ck, cv, cp, workspace=False) == "exact"
    assert not kf.tiling(*kf.SAVES_EXACT[1][:2]).full_w and kf.tiling(*kf.SAVES_EXACT[0][:2]).tiles == 1
    forms = {kf.CASES[c][2] for c in kf.SAVES_BF16}                    # both two-sub-tile forms are anchored in their one-tile version,
    assert forms == {"pair", "packed56"} and any(not kf.tiling(*kf.CASES[c][0]).full_w for c in kf.SAVES_BF16 + kf.SAVES_SPLIT)    # column-tiled too
    assert kf.arm("fp32", 64, 256, 512) == "exact"                     # (two images of 64 x 848 bf16 do not fit the LDS)
    with pytest.raises(ValueError):
        kf.bf16_form(1, 256, 64, 1280)


def test_bwd_pre_trip_counts():
    trips = [kf.bwd_pre_trips(bt * n, cp) for bt, n, cp in kf.PRE_CASES]
    assert [(t.trips, t.partial) for t in trips] == [(1, True), (2, True), (7, True)]
    assert kf.PRE_CASES[1][:2] == (257, 49)
    # every backward test of tests/test_backward_gpu.py's small batches stays on one trip
    assert kf.bwd_pre_trips(3 * 49, 256).trips == 1 and kf.bwd_pre_trips(3 * 6 * 19, 64).trips == 1 and kf.bwd_pre_trips(2 * 14 * 14, 128).trips == 1
    for cus in CU_COUNTS:                                              # the whole-op backward at the threshold: a takes 2, e takes 9
        trips = {}
        for case in kf.BACKWARD_BF16:
            (h, w), (ck, cv, cp), _, odd = kf.CASES[case]
            trips[case] = kf.bwd_pre_trips(kf.threshold_bt(h, w, cus, odd) * h * w, cp).trips
        assert trips == {"a": 2, "e": 9, "f": 1}


def test_projection_case_takes_128_row_tiles():
    rows, k, widths = kf.PROJ_CASE
    assert rows >= kf.PROJ_TM_SWITCH == 128 * 512 and kf.proj_tile(rows) == 128 and rows % 128 == 77 and rows % 16 != 0
    assert kf.proj_tile(kf.PROJ_TM_SWITCH - 1) == 64 and kf.proj_tile(25088) == 64 and k % 32 == 0 and all(x % 16 == 0 for x in widths)


# ------------------------------------------------------------------------------------------------------------------ (c)
def _qdiv(n, d):
    """(int)(((float)n + 0.5f) * inv) with inv = 1.0f / d, in float32 as the kernel evaluates it."""
    inv = np.float32(1.0) / np.float32(d)
    return ((n.astype(np.float32) + np.float32(0.5)) * inv).astype(np.int32)


def test_float_reciprocal_divisions_are_exact_for_the_cases():
    """kpff_bf16_kernel: gtok's tok -> row of the tile (tile widths of the column-tiled grids) and the staging's idx -> tile row."""
    tok = np.arange(kf.KPFF_TM, dtype=np.int32)
    for width in range(1, kf.COL_TILE_COLS + 1):
        assert np.array_equal(_qdiv(tok, width), tok // width)
    for (h, w), (ck, cv, cp), _, _ in kf.CASES.values():
        q8 = (cp + ck) // 8
        idx = np.arange(2 * kf.KPFF_TM * q8 + 4 * 512, dtype=np.int32)
        assert np.array_equal(_qdiv(idx, q8), idx // q8)
