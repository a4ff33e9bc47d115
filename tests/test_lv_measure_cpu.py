"""CPU checks of the LV measurement: known answers of the reference (tests/lv_reference.py restates include/gdkvm.h), the wrappers' refusals,
the configuration key and the statistics derived from ops.ef_summary."""
import math
import os

import numpy as np
import pytest
import torch

from tests import lv_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = R.Q
RECTS = [(40, 12), (50, 12), (16, 16), (7, 3), (1, 1)]                      # (w, h)
ELLIPSES = [(112, 40, 18), (256, 90, 40), (1024, 480, 300)]                  # (frame side, long semi-axis, short semi-axis)


def _rect(H, W, y0, x0, h, w, cls=1):
    m = np.zeros((H, W), np.uint8)
    m[y0:y0 + h, x0:x0 + w] = cls
    return m


def _sum_identity(res, D):
    n = res["stats"][0]
    assert sum(res["disks"]) == n * D * n * Q


@pytest.mark.parametrize("w,h", RECTS)
def test_rectangle_volume_is_the_cylinder(w, h):
    """An axis-aligned w x h rectangle measured along y is a stack of equal disks of diameter w: V = pi w^2 h / 4, whatever h mod D."""
    for D in (20, 7):
        res = R.lv_measure_ref(_rect(64, 64, 5, 9, h, w), 1, D, axis=(0, Q))
        assert res["geom"][1] == pytest.approx(math.pi * w * w * h / 4.0, rel=1e-12)
        assert res["geom"][0] == pytest.approx(float(h), rel=1e-12)
        assert res["stats"][0] == w * h
        _sum_identity(res, D)
        # the transpose measured along x
        res = R.lv_measure_ref(_rect(64, 64, 9, 5, w, h), 1, D, axis=(Q, 0))
        assert res["geom"][1] == pytest.approx(math.pi * w * w * h / 4.0, rel=1e-12)
        _sum_identity(res, D)


def test_axis_found_from_the_moments():
    # a square has no preferred direction (r == 0): the default is the image's vertical
    res = R.lv_measure_ref(_rect(40, 40, 3, 7, 16, 16))
    assert res["stats"][6:8] == [0, Q]
    assert res["geom"][1] == pytest.approx(math.pi * 16 * 16 * 16 / 4.0, rel=1e-12)
    assert res["geom"][2:] == [7 + 7.5, 3 + 7.5]
    _sum_identity(res, 20)
    # the longer side wins, in either orientation
    tall = R.lv_measure_ref(_rect(64, 64, 2, 3, 40, 12))
    assert tall["stats"][6:8] == [0, Q] and tall["geom"][1] == pytest.approx(math.pi * 12 * 12 * 40 / 4.0, rel=1e-12)
    wide = R.lv_measure_ref(_rect(64, 64, 2, 3, 12, 40))
    assert wide["stats"][6:8] == [Q, 0] and wide["geom"][1] == pytest.approx(math.pi * 12 * 12 * 40 / 4.0, rel=1e-12)
    # a 45-degree diagonal line: A == C, B != 0
    d = np.zeros((20, 20), np.uint8)
    d[np.arange(3, 15), np.arange(2, 14)] = 1
    res = R.lv_measure_ref(d)
    assert res["stats"][6] == res["stats"][7] == round(Q / math.sqrt(2.0))
    _sum_identity(res, 20)
    # other classes and the ignore label are "not cls"; an empty frame is all zeros
    m = _rect(32, 32, 4, 4, 10, 5)
    m[20:, :] = 255
    m[0, :] = 2
    assert R.lv_measure_ref(m)["stats"][0] == 50 and R.lv_measure_ref(m, cls=2)["stats"][0] == 32
    assert R.lv_measure_ref(m, cls=3) == {"stats": [0] * 12, "disks": [0] * 20, "geom": [0.0] * 4}


@pytest.mark.parametrize("S,la,sa", ELLIPSES)
def test_rasterised_ellipse_is_close_to_the_prolate_spheroid(S, la, sa):
    want = 4.0 / 3.0 * math.pi * la * sa * sa
    for deg in (0, 30, 45, 90):
        res = R.lv_measure_ref(R.ellipse_mask(S, S, S / 2 - 0.5, S / 2 - 0.5, la, sa, deg))
        assert abs(res["geom"][1] - want) <= 0.01 * want, (deg, res["geom"][1] / want)
        _sum_identity(res, 20)


def test_ef_reference():
    vol = [[3.0, 9.0, 9.0, 1.0, 1.0], [5.0, 0.0, 7.0, 2.0, 2.0], [1.0, 2.0, 3.0, 4.0, 5.0], [0.0, 0.0, 0.0, 0.0, 0.0]]
    npx = [[5, 5, 5, 5, 5], [5, 0, 5, 0, 0], [0, 0, 4, 0, 0], [3, 3, 0, 0, 0]]
    idx, val = R.lv_ef_ref(vol, npx)
    assert idx == [[1, 3, 5], [2, 0, 2], [-1, -1, 1], [0, 0, 2]]            # ties -> lowest t; one valid frame -> none; EDV == 0 -> EF 0
    assert val[0] == [9.0, 1.0, 8.0 / 9.0] and val[1] == [7.0, 5.0, 2.0 / 7.0] and val[2] == [0.0] * 3 and val[3] == [0.0] * 3
    idx, val = R.lv_ef_ref(vol, npx, min_pixels=5)
    assert idx[2] == [-1, -1, 0] and idx[3] == [-1, -1, 0]
    pick = [[1.0, 2.0, 3.0, 4.0, 5.0]] * 4
    idx, val = R.lv_ef_ref(vol, npx, pick_vol=pick, pick_npix=[[1] * 5] * 4)
    assert idx[0] == [4, 0, 5] and val[0] == [1.0, 3.0, -2.0]


def test_no_cpu_fallback_and_wrapper_refusals():
    from gdkvm_amd import build, ops
    build.build()
    m = torch.zeros(2, 8, 8, dtype=torch.uint8)
    with pytest.raises(ops.GdkvmError, match="device"):
        ops.lv_measure(m)
    with pytest.raises(ops.GdkvmError, match="device"):
        ops.lv_ef(torch.zeros(2, 4, dtype=torch.float64), torch.zeros(2, 4, dtype=torch.int64))
    with pytest.raises(ops.GdkvmError, match="uint8"):
        ops.lv_measure(m.float())
    with pytest.raises(ops.GdkvmError, match="uint8"):
        ops.lv_measure(torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(ops.GdkvmError, match="1..1024"):
        ops.lv_measure(torch.zeros(1, 2, 1025, dtype=torch.uint8))
    with pytest.raises(ops.GdkvmError, match="disks"):
        ops.lv_measure(m, disks=65)
    with pytest.raises(ops.GdkvmError, match="disks"):
        ops.lv_measure(m, disks=0)
    with pytest.raises(ops.GdkvmError, match="cls"):
        ops.lv_measure(m, cls=255)
    v, n = torch.zeros(2, 4, dtype=torch.float64), torch.zeros(2, 4, dtype=torch.int64)
    with pytest.raises(ops.GdkvmError, match="together"):
        ops.lv_ef(v, n, pick_vol=v)
    with pytest.raises(ops.GdkvmError, match="vol must be"):
        ops.lv_ef(v[0], n[0])
    with pytest.raises(ops.GdkvmError, match="npix must be"):
        ops.lv_ef(v, n.int())
    with pytest.raises(ops.GdkvmError, match="vol must be"):
        ops.lv_ef(v.float(), n)
    with pytest.raises(ops.GdkvmError, match="pick_npix must be"):
        ops.lv_ef(v, n, pick_vol=v, pick_npix=n[:, :3])


def test_c_entry_points_refuse_bad_arguments():
    """The argument checks of the C calls sit in front of anything that needs a device."""
    import ctypes
    from gdkvm_amd import build, ops
    build.build()
    lib = ops.load()
    buf = (ctypes.c_uint8 * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    ok = lambda **kw: dict(dict(mask=p, stats=p, disks=p, geom=p, frames=1, H=8, W=8, cls=1, D=20), **kw)
    call = lambda a: lib.gdkvm_lv_measure(a["mask"], a["stats"], a["disks"], a["geom"], a["frames"], a["H"], a["W"], a["cls"], a["D"], None)
    assert call(ok(frames=0)) == 0 and call(ok(frames=0, mask=None)) == 0
    for bad in (dict(H=0), dict(W=1025), dict(H=1025), dict(D=0), dict(D=65), dict(frames=-1)):
        assert call(ok(**bad)) == -1, bad
    for bad in (dict(cls=-1), dict(cls=255), dict(mask=None), dict(stats=None), dict(disks=None), dict(geom=None), dict(stats=p + 8),
                dict(disks=p + 8), dict(geom=p + 8)):
        assert call(ok(**bad)) == -6, bad
    assert b"16-byte" in lib.gdkvm_last_error()
    ef = lambda vol=p, npix=p, pv=None, pn=None, idx=p, val=p, B=1, T=4: lib.gdkvm_lv_ef(vol, npix, pv, pn, idx, val, B, T, 1, None)
    assert ef(B=0) == 0
    assert ef(T=0) == -1 and ef(B=-1) == -1
    assert ef(pv=p) == -6 and ef(pn=p) == -6 and ef(vol=None) == -6 and ef(idx=None) == -6 and ef(idx=p + 4) == -6 and ef(val=p + 8) == -6
    assert ef(vol=p + 4) == -6


def test_lv_class_config_key():
    from gdkvm_amd.config import load_config
    path = os.path.join(ROOT, "config", "config_gdkvm_01.yaml")
    assert load_config(path).data.lv_class == 1 and load_config(None, []).data.lv_class == 1
    assert load_config(path, ["data.lv_class=-1"]).data.lv_class == -1
    assert load_config(path, ["data.lv_class=2"]).data.lv_class == 2


def test_iou_and_ef_statistics_agree_with_numpy():
    from gdkvm_amd import ops
    counts = torch.tensor([[50, 60, 70], [0, 0, 0], [0, 5, 9], [7, 7, 7]])
    c = counts.numpy().astype(np.float64)
    want = (c[:, 0] + 1e-6) / (c[:, 1] + c[:, 2] - c[:, 0] + 1e-6)
    got = ops.iou_from_counts(counts)
    assert got.dtype == torch.float64 and np.allclose(got.numpy(), want, rtol=1e-15, atol=0)
    assert got[1] == 1.0 and got[3] == 1.0 and got[2] < 1e-6
    p = np.array([0.61, 0.55, 0.32, 0.48, 0.70, 0.12, 0.66])
    g = np.array([0.58, 0.60, 0.35, 0.41, 0.72, 0.90, 0.59])
    ok = np.array([1, 1, 1, 1, 1, 0, 1], bool)
    s1 = ops.ef_summary(torch.from_numpy(p[:4]), torch.from_numpy(g[:4]), torch.from_numpy(ok[:4]))
    s2 = ops.ef_summary(torch.from_numpy(p[4:]), torch.from_numpy(g[4:]), torch.from_numpy(ok[4:]))
    assert s1.shape == (8,) and s1.dtype == torch.float64
    st = ops.ef_stats(s1 + s2)                                   # sums of batches (or ranks) add
    e = p[ok] - g[ok]
    assert st["clips_with_ef"] == 6
    assert st["ef_mae"] == pytest.approx(np.abs(e).mean(), rel=1e-12) and st["ef_bias"] == pytest.approx(e.mean(), rel=1e-12)
    assert st["ef_pearson_r"] == pytest.approx(np.corrcoef(p[ok], g[ok])[0, 1], rel=1e-10)
    assert st["mean_ref_ef"] == pytest.approx(g[ok].mean(), rel=1e-12) and st["mean_pred_ef"] == pytest.approx(p[ok].mean(), rel=1e-12)
    assert ops.ef_stats(torch.zeros(8))["clips_with_ef"] == 0 and ops.ef_stats(torch.zeros(8))["ef_pearson_r"] == 0.0
