"""CPU checks of the surface distances: the reference (tests/surface_reference.py restates include/gdkvm.h) against known answers and against
scipy by the medpy recipe, the torch helpers on top of the integer record (ops.surface_metrics / surface_summary / surface_stats) against the
reference's floats, the refusals of the wrapper and of the C entry point, and the configuration key."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import surface_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 65536


def _z(H=40, W=40):
    return np.zeros((H, W), np.uint8)


def test_known_answers():
    a, b = _z(), _z()
    a[10:30, 8:24] = 1
    b[10:30, 13:29] = 1                                          # A shifted 5 columns right
    rec = S.surface_distance_ref(a, b)
    assert rec == [68, 68, 25, 25, 12451840, 12451840, 25, 25]   # 38 pixels per direction at distance 5: 38 * 5 * 65536
    hd, hd95, assd, valid = S.metrics_ref(rec)
    assert valid and hd == 5.0 and hd95 == 5.0 and assd == 190 / 68
    a, b = _z(), _z()
    a[0, 0] = 1; b[39, 39] = 1
    assert S.surface_distance_ref(a, b) == [1, 1, 3042, 3042, 3614594, 3614594, 3042, 3042]
    assert 3614594 == math.isqrt(3042 << 32)
    a, b = np.ones((40, 40), np.uint8), _z()
    b[20, 20] = 1
    assert S.surface_distance_ref(a, b) == [156, 1, 800, 361, 228913306, 1245184, 724, 724]
    a = _z(); a[5:20, 7:31] = 1; a[25:30, 3:9] = 1
    rec = S.surface_distance_ref(a, a.copy())
    assert rec[0] == rec[1] > 0 and rec[2:] == [0] * 6 and S.metrics_ref(rec) == (0.0, 0.0, 0.0, True)
    assert S.surface_distance_ref(_z(), a) == [0, rec[1], 0, 0, 0, 0, 0, 0]
    assert S.surface_distance_ref(a, _z()) == [rec[0], 0, 0, 0, 0, 0, 0, 0]
    assert S.surface_distance_ref(_z(), _z()) == [0] * 8 and S.metrics_ref([0] * 8) == (0.0, 0.0, 0.0, False)


def test_other_bytes_are_not_the_class_and_wraps_are_no_adjacency():
    a = np.full((6, 7), 255, np.uint8)
    a[1:5, 1:6] = 2; a[2, 2] = 1
    b = np.full((6, 7), 3, np.uint8); b[4, 5] = 1
    assert S.surface_distance_ref(a, b, cls=1)[:4] == [1, 1, 13, 13]
    assert S.surface_distance_ref(a, a, cls=2)[:2] == [16, 16]   # 20 - 1 pixels; (2, 4), (3, 3) and (3, 4) keep their four neighbours
    # (W - 1, y) and (0, y + 1) follow each other in memory and are no neighbours: a full 3 x 3 block has ONE inner pixel, a row of 9 none
    m = np.ones((3, 3), np.uint8)
    assert int(S.surface(m == 1).sum()) == 8 and int(S.surface(np.ones((1, 9), bool)).sum()) == 9
    lat = S.lattice(40, 45)
    assert int(S.surface(lat == 1).sum()) == int((lat == 1).sum()) and int((lat == 1).sum()) * 5 == 4 * 40 * 45


@pytest.mark.parametrize("H,W", [(112, 112), (30, 58), (15, 13), (8, 1024), (1, 37), (37, 1), (128, 144)])
def test_reference_agrees_with_scipy(H, W):
    """medpy's recipe written out: border = X ^ binary_erosion(X, cross, border_value 0); distances = distance_transform_edt(~other border) at this
    border; hd = max of both maxima, hd95 = np.percentile(hstack, 95), assd = mean of the two directed means.  Every shape compares all six
    cases (three frame pairs, classes 1 and 2): the one-pixel-wide shapes use random runs along the line, where an ellipse has no room."""
    from scipy import ndimage
    cross = ndimage.generate_binary_structure(2, 1)
    frames = (S.random_frames if min(H, W) >= 8 else S.run_frames)(6, H, W, seed=H * 31 + W)
    compared = 0
    for k in range(3):
        for cls in (1, 2):
            m, t = frames[2 * k], frames[2 * k + 1]
            A, B = m == cls, t == cls
            assert A.any() and B.any(), (k, cls)
            SA, SB, dab, dba = S.directed(m, t, cls)
            ba, bb = A ^ ndimage.binary_erosion(A, structure=cross, iterations=1), B ^ ndimage.binary_erosion(B, structure=cross, iterations=1)
            assert np.array_equal(SA, ba) and np.array_equal(SB, bb)
            ea, eb = ndimage.distance_transform_edt(~bb)[ba], ndimage.distance_transform_edt(~ba)[bb]
            assert np.array_equal(np.rint(ea * ea).astype(np.int64), dab) and np.array_equal(np.rint(eb * eb).astype(np.int64), dba)
            rec = S.surface_distance_ref(m, t, cls)
            hd, hd95, assd, valid = S.metrics_ref(rec)
            assert valid
            assert hd == pytest.approx(max(ea.max(), eb.max()), rel=1e-12, abs=0)
            assert hd95 == pytest.approx(np.percentile(np.hstack((ea, eb)), 95), rel=1e-12, abs=0)
            # scipy's distances averaged in exact rationals against the record's exact ASSD: every term of the record is rounded down by less
            # than 2^-16 pixel, so the difference lies in [0, 2^-16) -- no rounding of a sum or a mean enters the lower bound
            exact = lambda d: sum(Fraction(float(v)) for v in d) / len(d)
            gap = (exact(ea) + exact(eb)) / 2 - (Fraction(rec[4], rec[0]) + Fraction(rec[5], rec[1])) / 2 / Q
            assert 0 <= gap and gap < 2.0 ** -16 + 1e-12, float(gap)
            assert abs(float((Fraction(rec[4], rec[0]) + Fraction(rec[5], rec[1])) / 2 / Q) - assd) <= 1e-12 * max(assd, 1.0)
            compared += 1
    assert compared == 6


def _records():
    frames = S.random_frames(8, 30, 58, seed=5)
    rec = S.surface_distance_frames(frames[:4], frames[4:], 1)
    extra = np.asarray([[0, 7, 0, 0, 0, 0, 0, 0], [9, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0], [1, 1, 3042, 3042, 3614594, 3614594, 3042, 3042],
                        [156, 1, 800, 361, 228913306, 1245184, 724, 724], [3, 4, 10, 17, 5 * Q, 9 * Q, 9, 16]], np.int64)
    return np.concatenate([rec, extra])


def test_surface_metrics_summary_and_stats_on_cpu_tensors():
    from gdkvm_amd import ops
    rec = _records()
    surf = torch.from_numpy(rec)
    met, valid = ops.surface_metrics(surf)
    assert met.dtype == torch.float64 and met.shape == (10, 3) and valid.dtype == torch.bool and valid.shape == (10,)
    want = [S.metrics_ref(r) for r in rec]
    assert valid.tolist() == [w[3] for w in want] and valid.tolist()[4:7] == [False] * 3
    for got, w in zip(met.tolist(), want):
        assert got == pytest.approx(list(w[:3]), rel=1e-14, abs=0)
    assert met[9].tolist() == pytest.approx([math.sqrt(17), 3 + 0.7 * (4 - 3), (5 / 3 + 9 / 4) / 2], rel=1e-14)      # n = 7: 95 * 6 = 570 -> rank 5, fraction 0.7
    m2, v2 = ops.surface_metrics(surf.view(2, 5, 8))                                 # leading dimensions are kept
    assert m2.shape == (2, 5, 3) and v2.shape == (2, 5) and torch.equal(m2.view(10, 3), met)
    labelled = torch.tensor([True, True, False, True, True, True, False, True, True, False])
    sums = ops.surface_summary(met, valid, surf, labelled)
    assert sums.dtype == torch.float64 and sums.shape == (5,)
    rows = [i for i in range(10) if labelled[i] and want[i][3]]
    assert rows == [0, 1, 3, 7, 8]
    assert sums.tolist() == pytest.approx([5, 2] + [math.fsum(want[i][k] for i in rows) for k in range(3)], rel=1e-14)
    both = ops.surface_summary(m2, v2, surf.view(2, 5, 8), labelled.view(2, 5))
    assert both.tolist() == pytest.approx(sums.tolist(), rel=1e-14)
    st = ops.surface_stats(sums)
    assert list(st) == ["frames", "frames_one_empty", "hd_mean", "hd95_mean", "assd_mean"] and st["frames"] == 5 and st["frames_one_empty"] == 2
    assert [st["hd_mean"], st["hd95_mean"], st["assd_mean"]] == pytest.approx([float(sums[k]) / 5 for k in (2, 3, 4)], rel=1e-15)
    assert st["assd_mean"] <= st["hd95_mean"] <= st["hd_mean"]
    assert ops.surface_stats(torch.zeros(5)) == {"frames": 0, "frames_one_empty": 0, "hd_mean": 0.0, "hd95_mean": 0.0, "assd_mean": 0.0}
    with pytest.raises(ops.GdkvmError, match="surf"):
        ops.surface_metrics(torch.zeros(3, 7, dtype=torch.int64))
    with pytest.raises(ops.GdkvmError, match="surf"):
        ops.surface_metrics(torch.zeros(3, 8))


def test_no_cpu_fallback_and_wrapper_refusals():
    from gdkvm_amd import build, ops
    build.build()
    m = torch.zeros(2, 8, 8, dtype=torch.uint8)
    with pytest.raises(ops.GdkvmError, match="device"):
        ops.surface_distance(m, m)
    with pytest.raises(ops.GdkvmError, match="uint8"):
        ops.surface_distance(m.float(), m)
    with pytest.raises(ops.GdkvmError, match="target must be"):
        ops.surface_distance(m, m.int())
    with pytest.raises(ops.GdkvmError, match="target must be"):
        ops.surface_distance(m, m[:1])
    with pytest.raises(ops.GdkvmError, match="cls"):
        ops.surface_distance(m, m, cls=255)
    with pytest.raises(ops.GdkvmError, match="cls"):
        ops.surface_distance(m, m, cls=-1)
    big = torch.zeros(1, 2, 1025, dtype=torch.uint8)
    with pytest.raises(ops.GdkvmError, match="1..1024"):
        ops.surface_distance(big, big)


def test_c_entry_point_refuses_bad_arguments():
    """Every bad argument is GDKVM_ERR_SHAPE, in front of anything that needs a device; the workspace is 0 while the frame lives in LDS."""
    import ctypes
    from gdkvm_amd import build, ops
    build.build()
    lib = ops.load()
    need = lib.gdkvm_surface_distance_workspace_bytes
    assert need(4, 112, 112) == 0 and need(1, 112, 128) == 0                         # up to 14336 pixels
    words = lambda hw: (((hw + 3) // 4 * 4) + 4 * (((hw + 31) // 32 + 3) // 4 * 4) + 31) // 32 * 32
    assert need(2, 113, 127) == 2 * 4 * words(113 * 127) and need(2, 256, 256) == 2 * 4 * words(65536) == 2 * 294912
    assert need(3, 1024, 1024) == 3 * 4 * words(1 << 20) == 3 * 4718592
    assert need(0, 256, 256) == 0 and need(1, 1025, 8) == 0 and need(-1, 8, 8) == 0
    buf = (ctypes.c_uint8 * 8192)()
    p = (ctypes.addressof(buf) + 15) & ~15
    big = 2 * 294912
    ok = lambda **kw: dict(dict(mask=p, target=p, surf=p, ws=None, wsb=0, frames=1, H=8, W=8, cls=1), **kw)
    call = lambda a: lib.gdkvm_surface_distance(a["mask"], a["target"], a["surf"], a["ws"], a["wsb"], a["frames"], a["H"], a["W"], a["cls"], None)
    assert call(ok(frames=0)) == 0 and call(ok(frames=0, mask=None, target=None, surf=None)) == 0
    bads = (dict(H=1025), dict(W=1025), dict(H=0), dict(W=0), dict(frames=-1), dict(cls=255), dict(cls=-1), dict(mask=None), dict(target=None),
            dict(surf=None), dict(surf=p + 8), dict(frames=2, H=256, W=256, ws=p, wsb=big - 1), dict(frames=2, H=256, W=256, ws=None, wsb=big),
            dict(frames=2, H=256, W=256, ws=p + 4, wsb=big))
    for bad in bads:
        assert call(ok(**bad)) == -1, bad
        assert lib.gdkvm_last_error().startswith(b"surface_distance:"), bad
    assert call(ok(frames=0, cls=255)) == -1                                         # the checks come before the frames == 0 shortcut


def test_surface_class_config_key():
    from gdkvm_amd.config import load_config
    path = os.path.join(ROOT, "config", "config_gdkvm_01.yaml")
    assert load_config(path).data.surface_class == -1 and load_config(None, []).data.surface_class == -1
    assert load_config(path, ["data.surface_class=1"]).data.surface_class == 1
    assert load_config(path, ["data.surface_class=0"]).data.surface_class == 0
    assert load_config(path, ["data.surface_class=3"]).data.surface_class == 3
    assert load_config(path, ["data.surface_class=-1"]).data.surface_class == -1
    for bad in ("4", "-2", "true", "one", "1.0"):
        with pytest.raises(ValueError, match="surface_class"):
            load_config(path, [f"data.surface_class={bad}"])
    with pytest.raises(ValueError, match="surface_class"):
        load_config(path, ["data.num_classes=2", "data.surface_class=2"])
