"""CPU checks of the hole filling: the reference (tests/holes_reference.py restates include/gdkvm.h) against scipy where it is installed and
against known answers on hand-drawn frames, class_counts_after_fill against counts recomputed from the filled mask, the two configuration
keys, the refusals of the wrapper and of the C entry point, and the example the feature exists for: a hole that moves the LV measurement."""
import os

import numpy as np
import pytest
import torch

from tests import cc_reference as C
from tests import holes_reference as Hr
from tests import lv_reference as R
from tests.test_largest_component_gpu import _random_frames, _special_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCIPY_SHAPES = [(112, 112), (30, 58), (15, 13), (8, 1024), (1, 37), (1, 1)]


def _ellipse(la=40, sa=18):
    return R.ellipse_mask(112, 112, 56, 56, la, sa, 20)


def _frames(H, W, cls):
    fr = list(_random_frames(2, H, W, seed=H * 1000 + W)) + list(_special_frames(H, W, cls, seed=H + W))
    if H >= 13 and W >= 13:
        fr += list(Hr.hand_frames(H, W, cls).values()) + [Hr.plugged_spiral(H, W, cls)]
    return fr


@pytest.mark.parametrize("connectivity", [4, 8])
def test_reference_agrees_with_scipy(connectivity):
    """The filled mask against binary_fill_holes, the holes and their sizes against label() of what it filled."""
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2)
    seen = 0
    for H, W in SCIPY_SHAPES:
        for cls in (1, 2):
            for m in _frames(H, W, cls):
                filled = ndimage.binary_fill_holes(m == cls, structure=structure)
                out, info = Hr.fill_holes_ref(m, cls, connectivity, 0)
                assert np.array_equal(out == cls, filled) and np.array_equal(out[~filled], m[~filled])
                lab, k = ndimage.label(filled & (m != cls), structure=structure)
                sizes = np.bincount(lab.ravel())[1:]
                assert info[:5] == [k, k, int((m == cls).sum()), int(sizes.sum()), int(sizes.max()) if k else 0], (H, W, cls)
                assert sorted(Hr.hole_labels(m, cls, connectivity)[1].values()) == sorted(sizes.tolist())
                cap = Hr.fill_holes_ref(m, cls, connectivity, 4)[1]
                assert cap[:5] == [k, int((sizes <= 4).sum()), info[2], int(sizes[sizes <= 4].sum()), info[4]]
                seen += k
    assert seen > 100                                              # the comparison is not vacuous: the frames do have holes


def test_known_answers_on_hand_drawn_frames():
    fr = Hr.hand_frames(15, 17)
    info = lambda name, conn, area=0: Hr.fill_holes_ref(fr[name], 1, conn, area)[1][:5]
    n = lambda name: int((fr[name] == 1).sum())
    # a hole that leaks only diagonally is a hole at 4 and none at 8
    assert info("diagonal leak", 4) == [1, 1, n("diagonal leak"), 9, 9] and info("diagonal leak", 8) == [0, 0, n("diagonal leak"), 0, 0]
    # two holes that touch diagonally: two of 4 pixels at 4, one of 8 pixels at 8 -- max_area = 4 tells them apart
    assert info("diagonal holes", 4, 4) == [2, 2, 28, 8, 4] and info("diagonal holes", 8, 4) == [1, 0, 28, 0, 8]
    assert info("diagonal holes", 8) == [1, 1, 28, 8, 8]
    for conn in (4, 8):
        out, i = Hr.fill_holes_ref(fr["notch"], 1, conn)
        assert i == [0, 0, 22, 0, 0, 0, 0, 0] and np.array_equal(out, fr["notch"])                  # open to the frame's edge: no hole
        out, i = Hr.fill_holes_ref(fr["border frame"], 1, conn)
        assert i[:5] == [1, 1, 2 * 15 + 2 * 17 - 4, 13 * 15, 13 * 15] and (out == 1).all()           # the whole interior is one hole
        out, i = Hr.fill_holes_ref(fr["nested"], 1, conn)
        want = np.zeros((15, 17), np.uint8); want[1:12, 1:12] = 1
        assert i[:5] == [2, 2, 121 - 81 + 24, 57, 56] and np.array_equal(out, want)                 # both holes filled, the island kept
        out, i = Hr.fill_holes_ref(fr["ring"], 1, conn, 4)
        assert i[:5] == [4, 3, 121 - 29, 4, 25] and (out[4:9, 4:9] == 0).all() and int((out == 1).sum()) == 121 - 25
        assert Hr.fill_holes_ref(fr["ring"], 1, conn, 25)[1][:5] == [4, 4, 92, 29, 25]
        out, i = Hr.fill_holes_ref(fr["other bytes"], 1, conn)
        assert i[:5] == [1, 1, 24, 25, 25] and (out[1:8, 1:8] == 1).all() and int((out == 1).sum()) == 49
        sp = Hr.plugged_spiral(40, 51)
        out, i = Hr.fill_holes_ref(sp, 1, conn)
        assert i[0] == 1 and i[3] == i[4] == int((sp == 0).sum()) > 38 * 49 // 3 and (out == 1).all()
        # one-pixel-wide and two-pixel-wide frames never have holes; nor do an empty and a full frame
        for shape in ((1, 37), (37, 1), (2, 40), (40, 2), (1, 1)):
            m = np.zeros(shape, np.uint8); m[::2, ::3] = 1
            assert Hr.fill_holes_ref(m, 1, conn)[1][:2] == [0, 0] and Hr.fill_holes_ref(m, 0, conn)[1][:2] == [0, 0]
        assert Hr.fill_holes_ref(np.zeros((9, 9), np.uint8), 1, conn)[1] == [0] * 8
        assert Hr.fill_holes_ref(np.ones((9, 9), np.uint8), 1, conn)[1] == [0, 0, 81, 0, 0, 0, 0, 0]


def test_row_wrap_is_no_adjacency_and_filling_is_idempotent():
    # the hole's pixel (2, 5) and the outside pixel (3, 0) are consecutive bytes of a 6-wide frame, not neighbours
    m = np.zeros((6, 6), np.uint8)
    m[1:4, 3:6] = 1; m[2, 4] = 0; m[0, :] = 1; m[:, 5] = 1; m[2, 5] = 0; m[1, 4:] = 1; m[3, 4:] = 1; m[2, 4] = 1; m[2, 3] = 1
    m = np.pad(m, ((0, 0), (0, 1)), constant_values=1)             # (2, 5) is now enclosed: row 2 = ... 1 1 [0] 1
    for conn in (4, 8):
        out, info = Hr.fill_holes_ref(m, 1, conn)
        assert info[:5] == [1, 1, int((m == 1).sum()), 1, 1] and out[2, 5] == 1
    rng = np.random.default_rng(5)
    for conn, area in ((4, 0), (8, 0), (4, 3), (8, 3)):
        m = (rng.random((40, 45)) < 0.6).astype(np.uint8)
        out, info = Hr.fill_holes_ref(m, 1, conn, area)
        again, info2 = Hr.fill_holes_ref(out, 1, conn, area)
        assert info[1] > 0 and np.array_equal(again, out) and info2[1] == info2[3] == 0 and info2[2] == info[2] + info[3]
        assert info2[0] == info[0] - info[1]                       # what was left open is still there


def test_class_counts_after_fill_on_cpu_tensors():
    from gdkvm_amd import ops
    rng = np.random.default_rng(3)
    F, H, W = 5, 24, 31
    other = rng.integers(0, 4, (F, H, W)).astype(np.uint8)
    other[rng.random((F, H, W)) < 0.1] = 255
    dense = rng.random((F, H, W)) < 0.7                            # the class is dense enough to enclose holes, of every other byte
    target = rng.integers(0, 3, (F, H, W)).astype(np.uint8)
    target[4] = 255                                                # an unlabelled frame
    for cls, conn, area in ((1, 4, 0), (2, 8, 0), (1, 8, 2), (0, 4, 0)):
        mask = np.where(dense, np.uint8(cls), other)
        out, info = Hr.fill_holes_frames(mask, cls, conn, area, target)
        assert info[:, 3].sum() > 0
        o, t = torch.from_numpy(out) == cls, torch.from_numpy(target) == cls
        want = torch.stack([(o & t).sum((1, 2)), o.sum((1, 2)), t.sum((1, 2))], -1)
        got = ops.class_counts_after_fill(torch.from_numpy(info))
        assert got.dtype == torch.int64 and got.shape == (F, 3) and torch.equal(got, want), (cls, conn, area)
        assert torch.equal(ops.class_counts_after_fill(torch.from_numpy(info).view(1, F, 8).long()), want.view(1, F, 3))
        none = Hr.fill_holes_frames(mask, cls, conn, area)[1]
        assert np.array_equal(none[:, :5], info[:, :5]) and not none[:, 5:].any()
    with pytest.raises(ops.GdkvmError, match="info"):
        ops.class_counts_after_fill(torch.zeros(3, 7, dtype=torch.int32))
    with pytest.raises(ops.GdkvmError, match="info"):
        ops.class_counts_after_fill(torch.zeros(3, 8))


def test_lv_fill_holes_config_keys():
    from gdkvm_amd.config import load_config
    path = os.path.join(ROOT, "config", "config_gdkvm_01.yaml")
    for cfg in (load_config(path), load_config(None, [])):
        assert cfg.data.lv_fill_holes == 0 and cfg.data.lv_fill_max_area == 0
    assert load_config(path, ["data.lv_fill_holes=4"]).data.lv_fill_holes == 4
    cfg = load_config(path, ["data.lv_fill_holes=8", "data.lv_fill_max_area=50", "data.lv_keep_largest=4"])
    assert (cfg.data.lv_fill_holes, cfg.data.lv_fill_max_area, cfg.data.lv_keep_largest) == (8, 50, 4)
    assert load_config(path, ["data.lv_class=-1", "data.lv_fill_holes=4"]).data.lv_fill_holes == 4       # inert there, not refused
    for bad in ("3", "6", "-1", "true", "four"):
        with pytest.raises(ValueError, match="lv_fill_holes"):
            load_config(path, [f"data.lv_fill_holes={bad}"])
    for bad in ("-1", "2.5", "true", "many"):
        with pytest.raises(ValueError, match="lv_fill_max_area"):
            load_config(path, [f"data.lv_fill_max_area={bad}"])


def test_no_cpu_fallback_and_wrapper_refusals():
    from gdkvm_amd import build, ops
    build.build()
    m = torch.zeros(2, 8, 8, dtype=torch.uint8)
    with pytest.raises(ops.GdkvmError, match="device"):
        ops.fill_holes(m)
    with pytest.raises(ops.GdkvmError, match="uint8"):
        ops.fill_holes(m.float())
    with pytest.raises(ops.GdkvmError, match="1..1024"):
        ops.fill_holes(torch.zeros(1, 2, 1025, dtype=torch.uint8))
    with pytest.raises(ops.GdkvmError, match="connectivity"):
        ops.fill_holes(m, connectivity=6)
    for bad in (-1, 2.5, True):
        with pytest.raises(ops.GdkvmError, match="max_area"):
            ops.fill_holes(m, max_area=bad)
    with pytest.raises(ops.GdkvmError, match="cls"):
        ops.fill_holes(m, cls=255)
    with pytest.raises(ops.GdkvmError, match="target must be"):
        ops.fill_holes(m, target=m[:1])
    with pytest.raises(ops.GdkvmError, match="out must be"):
        ops.fill_holes(m, out=m.int())


def test_c_entry_point_refuses_bad_arguments():
    """Every bad argument is GDKVM_ERR_SHAPE, in front of anything that needs a device."""
    import ctypes
    from gdkvm_amd import build, ops
    build.build()
    lib = ops.load()
    need = lib.gdkvm_fill_holes_workspace_bytes
    assert need(4, 112, 112) == 0 and need(1, 120, 128) == 0                       # labels in LDS up to 15360 pixels
    assert need(2, 121, 127) == 2 * 15368 * 4 and need(2, 256, 256) == 2 * 65536 * 4 and need(3, 1024, 1024) == 3 * 4 * 1024 * 1024
    assert need(0, 256, 256) == 0 and need(1, 1025, 8) == 0 and need(-1, 8, 8) == 0
    buf = (ctypes.c_uint8 * 8192)()
    p = (ctypes.addressof(buf) + 15) & ~15
    big = 2 * 65536 * 4
    ok = lambda **kw: dict(dict(mask=p, target=None, out=p, info=p, ws=None, wsb=0, frames=1, H=8, W=8, cls=1, conn=4, area=0), **kw)
    call = lambda a: lib.gdkvm_fill_holes(a["mask"], a["target"], a["out"], a["info"], a["ws"], a["wsb"], a["frames"], a["H"], a["W"],
                                          a["cls"], a["conn"], a["area"], None)
    assert call(ok(frames=0)) == 0 and call(ok(frames=0, mask=None, out=None, info=None)) == 0
    bads = (dict(conn=6), dict(conn=0), dict(area=-1), dict(H=1025), dict(W=1025), dict(H=0), dict(frames=-1),
            dict(cls=255), dict(cls=-1), dict(info=None), dict(mask=None), dict(out=None), dict(info=p + 8), dict(out=p + 16),
            dict(frames=2, H=256, W=256, ws=p, wsb=big - 1), dict(frames=2, H=256, W=256, ws=None, wsb=big),
            dict(frames=2, H=256, W=256, ws=p + 4, wsb=big))
    for bad in bads:
        assert call(ok(**bad)) == -1, bad
        assert lib.gdkvm_last_error().startswith(b"fill_holes:"), bad
    assert call(ok(frames=0, conn=6)) == -1 and call(ok(frames=0, area=-1)) == -1   # the checks come before the frames == 0 shortcut


def test_the_hole_that_moves_the_measurement_is_filled():
    """The issue's figures, re-derived: an ellipse of semi-axes (40, 18) at 20 degrees in a 112 x 112 frame, D = 20, with discs of class 0 cut
    into it.  The bounds are the rounding of the quoted figures (0.1 % of the volume, 0.001 of EF)."""
    clean = _ellipse()
    base = R.lv_measure_ref(clean)
    assert int(clean.sum()) == 2261 and base["geom"][1] == pytest.approx(54011.8, abs=0.05) and base["geom"][0] == pytest.approx(80.63, abs=0.005)
    for (cy, cx, r), dn, dV in (((56, 56, 2), -0.006, -0.013), ((56, 56, 4), -0.022, -0.047), ((70, 61, 5), -0.036, -0.070),
                                ((56, 56, 6), -0.050, -0.102)):
        holed = C.disc(clean.copy(), cy, cx, r, value=0)
        got = R.lv_measure_ref(holed)
        assert holed.sum() / clean.sum() - 1 == pytest.approx(dn, abs=0.0005)
        assert got["geom"][1] / base["geom"][1] - 1 == pytest.approx(dV, abs=0.0005)
        assert round(got["geom"][0], 2) == round(base["geom"][0], 2) == 80.63        # the long axis is unchanged
        for conn in (4, 8):
            out, info = Hr.fill_holes_ref(holed, 1, conn)
            assert np.array_equal(out, clean) and info[:5] == [1, 1, int(holed.sum()), int(clean.sum() - holed.sum()), int(clean.sum() - holed.sum())]
            assert R.lv_measure_ref(out) == base                                     # the plain ellipse's record, exactly
    # clip level: holes on one frame only
    es = _ellipse(32, 13)
    assert int(es.sum()) == 1311
    vol = lambda m: R.lv_measure_ref(m)["geom"][1]
    npx = [[int(clean.sum()), int(es.sum())]]
    ef = lambda a, b: R.lv_ef_ref([[vol(a), vol(b)]], npx)[1][0][2]
    hole = lambda m, r: C.disc(m.copy(), 56, 56, r, value=0)
    ef_clean = ef(clean, es)
    assert ef_clean == pytest.approx(0.580, abs=0.0005)
    assert ef(clean, hole(es, 4)) == pytest.approx(0.613, abs=0.0005)
    assert ef(clean, hole(es, 6)) == pytest.approx(0.650, abs=0.0005)
    assert ef(hole(clean, 6), es) == pytest.approx(0.533, abs=0.0005)
    assert ef(Hr.fill_holes_ref(hole(clean, 6))[0], Hr.fill_holes_ref(hole(es, 6))[0]) == ef_clean
