"""CPU checks of the largest-connected-component filter: the reference (tests/cc_reference.py restates include/gdkvm.h) against scipy where it is
installed and against known answers, counts_after_largest against counts recomputed from the filtered mask, the configuration key, the
refusals of the wrapper and of the C entry point, and the example the feature exists for: an island that moves the LV measurement."""
import os

import numpy as np
import pytest
import torch

from tests import cc_reference as C
from tests import lv_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ellipse(S=112, la=40, sa=18):
    return R.ellipse_mask(S, S, S / 2, S / 2, la, sa, 20)


def _ellipse_frames():
    """The ellipse alone and with each island of the issue's table, plus a second class and an ignore patch that must not connect anything."""
    frames = [_ellipse()]
    for cy, cx, r in ((2, 2, 0), (12, 12, 4), (12, 100, 6), (100, 15, 8)):
        frames.append(C.disc(_ellipse(), cy, cx, r))
    m = C.disc(_ellipse(), 12, 100, 6)
    m[10:14, 60:100] = 2                                         # a bridge of ANOTHER class between the ventricle's row range and the island
    m[100:, :] = 255
    frames.append(m)
    return frames


@pytest.mark.parametrize("connectivity", [4, 8])
def test_reference_agrees_with_scipy(connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), int) if connectivity == 8 else np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    noise = (np.random.default_rng(0).random((256, 256)) < 0.55).astype(np.uint8)
    for m in [noise] + _ellipse_frames():
        H, W = m.shape
        lab, k = ndimage.label(m == 1, structure=structure)
        lin = np.arange(H * W).reshape(H, W)
        mins = np.asarray(ndimage.minimum(lin, lab, index=np.arange(1, k + 1))).astype(np.int64).reshape(-1)
        want = np.where(lab > 0, mins[np.maximum(lab, 1) - 1], -1)
        got = C.label_components(m, 1, connectivity)
        assert np.array_equal(got, want)
        sizes = np.bincount(lab.ravel())[1:]
        best = max(range(k), key=lambda i: (sizes[i], -mins[i]))
        out, info = C.largest_component_ref(m, 1, connectivity, fill=0)
        assert info[:4] == [k, int((m == 1).sum()), int(sizes[best]), int(mins[best])]
        keep = want == mins[best]
        assert np.array_equal(out, np.where((m == 1) & ~keep, 0, m))
    info4 = C.largest_component_ref(noise, 1, connectivity)[1]
    assert info4[1] == 36062 and info4[0] == (2999 if connectivity == 4 else 120)          # (what default_rng(0) gives: a sanity figure)


def test_known_answers():
    out, info = C.largest_component_ref(C.serpentine(64, 64))
    assert info == [1, 2080, 2080, 0, 0, 0, 0, 0] and np.array_equal(out, C.serpentine(64, 64))
    sp = C.spiral(40, 51)
    assert C.largest_component_ref(sp)[1][:4] == [1, int(sp.sum()), int(sp.sum()), 0] and sp.sum() > 40 * 51 // 3
    cb = C.checkerboard(33, 35)
    out, info = C.largest_component_ref(cb, connectivity=4, fill=7)
    assert info == [578, 578, 1, 0, 0, 0, 0, 0]
    assert out[0, 0] == 1 and int((out == 7).sum()) == 577 and int((out == 1).sum()) == 1
    out, info = C.largest_component_ref(cb, connectivity=8)
    assert info == [1, 578, 578, 0, 0, 0, 0, 0] and np.array_equal(out, cb)
    # empty frame; a frame of other classes only
    z = np.zeros((5, 9), np.uint8)
    out, info = C.largest_component_ref(z)
    assert info == [0, 0, 0, -1, 0, 0, 0, 0] and np.array_equal(out, z)
    z[:] = 255; z[2] = 2
    assert C.largest_component_ref(z, cls=1)[1] == [0, 0, 0, -1, 0, 0, 0, 0]
    assert C.largest_component_ref(z, cls=2, fill=0)[1][:4] == [1, 9, 9, 18]


def test_row_wrap_and_frame_wrap_are_no_adjacency():
    # (W - 1, y) and (0, y + 1) are consecutive bytes, not neighbours -- at either connectivity
    m = np.zeros((4, 6), np.uint8)
    m[1, 5] = m[2, 0] = 1
    for conn in (4, 8):
        out, info = C.largest_component_ref(m, connectivity=conn)
        assert info[:4] == [2, 2, 1, 11] and out[1, 5] == 1 and out[2, 0] == 0
    # the last byte of a frame and the first byte of the next: frames are independent
    fr = np.zeros((2, 3, 5), np.uint8)
    fr[0, 2, 4] = fr[0, 0, 0] = 1
    fr[1, 0, 0] = fr[1, 0, 1] = fr[1, 2, 2] = 1
    out, info = C.largest_component_frames(fr, connectivity=8)
    assert info[:, :4].tolist() == [[2, 2, 1, 0], [2, 3, 2, 0]]
    assert out[0, 0, 0] == 1 and out[0, 2, 4] == 0 and out[1, 2, 2] == 0


def test_size_tie_goes_to_the_smallest_label_and_a_later_larger_blob_wins():
    m = np.zeros((12, 12), np.uint8)
    m[1:3, 8:10] = 1                                             # label 20: met first along the rows
    m[2:6, 2] = 1                                                # label 26: as large
    m[8:10, 5:7] = 1                                             # label 101
    out, info = C.largest_component_ref(m)
    assert info[:4] == [3, 12, 4, 20] and int((out == 1).sum()) == 4 and out[1, 8] == 1
    m[2:6, 2] = 0
    m[1:5, 2] = 1                                                # now label 14 < 20: the winner is NOT the first one a row-major scan completes
    out, info = C.largest_component_ref(m)
    assert info[:4] == [3, 12, 4, 14] and out[1, 2] == 1 and out[1, 8] == 0
    m[8:11, 5:7] = 1                                             # a later blob of 6 beats both
    assert C.largest_component_ref(m)[1][:4] == [3, 14, 6, 101]
    # two blobs that touch only diagonally: one component at 8, two at 4
    d = np.zeros((8, 8), np.uint8)
    d[1:3, 1:3] = 1; d[3:6, 3:6] = 1
    assert C.largest_component_ref(d, connectivity=8)[1][:4] == [1, 13, 13, 9]
    assert C.largest_component_ref(d, connectivity=4)[1][:4] == [2, 13, 9, 27]


def test_hit_counts_and_counts_after_largest_on_cpu_tensors():
    from gdkvm_amd import ops
    rng = np.random.default_rng(3)
    ncls, F, H, W = 4, 5, 24, 31
    mask = rng.integers(0, ncls, (F, H, W)).astype(np.uint8)
    mask[rng.random((F, H, W)) < 0.05] = 255
    target = rng.integers(0, ncls, (F, H, W)).astype(np.uint8)
    target[4] = 255                                              # an unlabelled frame
    for cls, fill, conn in ((1, 0, 4), (2, 3, 8), (1, 200, 4), (0, 1, 8)):
        out, info = C.largest_component_frames(mask, cls, conn, fill, target)
        removed = (mask == cls) & (out != mask)
        assert info[:, 4].tolist() == [int((target[f][removed[f]] == cls).sum()) for f in range(F)]
        assert info[:, 5].tolist() == [int((target[f][removed[f]] == fill).sum()) for f in range(F)]
        before = torch.from_numpy(np.stack([C.counts_ref(mask[f], target[f], ncls) for f in range(F)]))
        after = np.stack([C.counts_ref(out[f], target[f], ncls) for f in range(F)])
        got = ops.counts_after_largest(before, torch.from_numpy(info), cls, fill)
        assert got.dtype == before.dtype and np.array_equal(got.numpy(), after), (cls, fill, conn)
        got32 = ops.counts_after_largest(before.int().view(1, F, ncls, 3), torch.from_numpy(info).view(1, F, 8), cls, fill)
        assert got32.dtype == torch.int32 and np.array_equal(got32.numpy()[0], after)
    with pytest.raises(ops.GdkvmError, match="leading"):
        ops.counts_after_largest(torch.zeros(2, 4, 3, dtype=torch.int64), torch.zeros(3, 8, dtype=torch.int32), 1, 0)
    with pytest.raises(ops.GdkvmError, match="cls"):
        ops.counts_after_largest(torch.zeros(2, 4, 3, dtype=torch.int64), torch.zeros(2, 8, dtype=torch.int32), 4, 0)


def test_lv_keep_largest_config_key():
    from gdkvm_amd.config import load_config
    path = os.path.join(ROOT, "config", "config_gdkvm_01.yaml")
    assert load_config(path).data.lv_keep_largest == 0 and load_config(None, []).data.lv_keep_largest == 0
    assert load_config(path, ["data.lv_keep_largest=4"]).data.lv_keep_largest == 4
    assert load_config(path, ["data.lv_keep_largest=8"]).data.lv_keep_largest == 8
    for bad in ("3", "6", "-1", "true", "four"):
        with pytest.raises(ValueError, match="lv_keep_largest"):
            load_config(path, [f"data.lv_keep_largest={bad}"])


def test_no_cpu_fallback_and_wrapper_refusals():
    from gdkvm_amd import build, ops
    build.build()
    m = torch.zeros(2, 8, 8, dtype=torch.uint8)
    with pytest.raises(ops.GdkvmError, match="device"):
        ops.largest_component(m)
    with pytest.raises(ops.GdkvmError, match="uint8"):
        ops.largest_component(m.float())
    with pytest.raises(ops.GdkvmError, match="1..1024"):
        ops.largest_component(torch.zeros(1, 2, 1025, dtype=torch.uint8))
    with pytest.raises(ops.GdkvmError, match="connectivity"):
        ops.largest_component(m, connectivity=6)
    with pytest.raises(ops.GdkvmError, match="fill"):
        ops.largest_component(m, cls=1, fill=1)
    with pytest.raises(ops.GdkvmError, match="cls"):
        ops.largest_component(m, cls=255)
    with pytest.raises(ops.GdkvmError, match="target must be"):
        ops.largest_component(m, target=m[:1])
    with pytest.raises(ops.GdkvmError, match="out must be"):
        ops.largest_component(m, out=m.int())


def test_c_entry_point_refuses_bad_arguments():
    """Every bad argument is GDKVM_ERR_SHAPE, in front of anything that needs a device."""
    import ctypes
    from gdkvm_amd import build, ops
    build.build()
    lib = ops.load()
    need = lib.gdkvm_largest_component_workspace_bytes
    assert need(4, 112, 112) == 0 and need(1, 120, 128) == 0                       # labels in LDS up to 15360 pixels
    assert need(2, 121, 127) == 2 * 15368 * 4 and need(2, 256, 256) == 2 * 65536 * 4 and need(3, 1024, 1024) == 3 * 4 * 1024 * 1024
    assert need(0, 256, 256) == 0 and need(1, 1025, 8) == 0 and need(-1, 8, 8) == 0
    buf = (ctypes.c_uint8 * 8192)()
    p = (ctypes.addressof(buf) + 15) & ~15
    big = 2 * 65536 * 4
    ok = lambda **kw: dict(dict(mask=p, target=None, out=p, info=p, ws=None, wsb=0, frames=1, H=8, W=8, cls=1, conn=4, fill=0), **kw)
    call = lambda a: lib.gdkvm_largest_component(a["mask"], a["target"], a["out"], a["info"], a["ws"], a["wsb"], a["frames"], a["H"], a["W"],
                                                 a["cls"], a["conn"], a["fill"], None)
    assert call(ok(frames=0)) == 0 and call(ok(frames=0, mask=None, out=None, info=None)) == 0
    bads = (dict(conn=6), dict(conn=0), dict(fill=1), dict(fill=256), dict(fill=-1), dict(H=1025), dict(W=1025), dict(H=0), dict(frames=-1),
            dict(cls=255), dict(cls=-1), dict(info=None), dict(mask=None), dict(out=None), dict(info=p + 8), dict(out=p + 16),
            dict(frames=2, H=256, W=256, ws=p, wsb=big - 1), dict(frames=2, H=256, W=256, ws=None, wsb=big),
            dict(frames=2, H=256, W=256, ws=p + 4, wsb=big))
    for bad in bads:
        assert call(ok(**bad)) == -1, bad
        assert lib.gdkvm_last_error().startswith(b"largest_component:"), bad
    assert call(ok(frames=0, conn=6)) == -1                                          # the checks come before the frames == 0 shortcut


def test_the_island_that_moves_the_measurement_is_removed():
    """The issue's figures, re-derived: an ellipse of semi-axes (40, 18) at 20 degrees in a 112 x 112 frame, D = 20."""
    clean = _ellipse()
    base = R.lv_measure_ref(clean)
    assert base["geom"][0] == pytest.approx(80.6, abs=0.05)
    # (island, extra pixels, long axis with it, change of the volume): a single pixel moves the axis most and the volume least
    for (cy, cx, r), extra, L, dV in (((2, 2, 0), 0.0004, 110.0, -0.003), ((12, 12, 4), 0.022, 102.5, 0.005), ((12, 100, 6), 0.050, 87.6, 0.058),
                                      ((100, 15, 8), 0.087, 94.7, 0.141)):
        dirty = C.disc(clean.copy(), cy, cx, r)
        got = R.lv_measure_ref(dirty)
        assert dirty.sum() / clean.sum() - 1 == pytest.approx(extra, abs=0.002)
        assert got["geom"][0] == pytest.approx(L, abs=0.6) and got["geom"][1] / base["geom"][1] - 1 == pytest.approx(dV, abs=0.004)
        for conn in (4, 8):
            out, info = C.largest_component_ref(dirty, 1, conn, 0)
            assert np.array_equal(out, clean) and info[:4] == [2, int(dirty.sum()), int(clean.sum()), int(np.flatnonzero(clean.ravel())[0])]
            assert R.lv_measure_ref(out) == base                                     # the plain ellipse's record, exactly
    # clip level: the radius-6 island on the end-systolic frame only
    es = R.ellipse_mask(112, 112, 56, 56, 32, 13, 20)
    es_dirty = C.disc(es.copy(), 12, 100, 6)
    vol = lambda m: R.lv_measure_ref(m)["geom"][1]
    npx = [[int(clean.sum()), int(es.sum())]]
    ef = lambda a, b: R.lv_ef_ref([[vol(a), vol(b)]], npx)[1][0][2]
    ef_clean, ef_dirty = ef(clean, es), ef(clean, es_dirty)
    assert ef_clean == pytest.approx(0.580, abs=0.002) and ef_dirty == pytest.approx(0.451, abs=0.003)
    assert ef(C.largest_component_ref(clean)[0], C.largest_component_ref(es_dirty)[0]) == ef_clean
