"""gdkvm_fill_holes on the device against tests/holes_reference.py, bit for bit: the filled mask and all eight info integers.  The shapes sit
where the kernel can go wrong rather than at the workload's size: both sides of the LDS / workspace split (15360 pixels), frames whose H*W is
no multiple of 16 (every frame after the first starts unaligned), one- and two-pixel-wide frames, rows longer than a wave's vectors."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import cc_reference as C
from tests import holes_reference as Hr
from tests import lv_reference as R
from tests.test_largest_component_gpu import _random_frames, _special_frames

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (frames of the random recipe, H, W): the cfg2 mask; exactly the last LDS size and the first workspace size; one larger workspace shape;
# H*W = 1740 and 195 (unaligned frames with heads and tails); one long row per 64 lanes; shapes that cannot hold a hole
LAST_LDS, FIRST_WS = (2, 120, 128), (2, 121, 127)
SHAPES = [(6, 112, 112), LAST_LDS, FIRST_WS, (2, 256, 256), (4, 30, 58), (5, 15, 13), (2, 8, 1024), (3, 1, 37), (3, 37, 1), (3, 2, 40), (1, 1, 1)]
ALL = [(conn, cls, area) for conn in (4, 8) for cls in (1, 2) for area in (0, 4)]


def _combos(H, W):
    """Every combination below 20000 pixels; above, two that still cover both connectivities, classes and areas (the Python reference is what
    costs time)."""
    return ALL if H * W < 20000 else [(4, 1, 4), (8, 2, 0)]


def _frames(F, H, W, cls):
    """The recipe of the largest-component test (random frames, then one frame per corner of ITS definition: percolation noise, serpentine,
    spiral, checkerboard, the full and the empty frame, ...), the hand-drawn frames of the CPU test in the shape's corner, and a spiral
    corridor of complement plugged at its outer end."""
    fr = [_random_frames(F, H, W, seed=H * 1000 + W), _special_frames(H, W, cls, seed=H + W)]
    if H >= 13 and W >= 13:
        fr += [np.stack(list(Hr.hand_frames(H, W, cls).values())), Hr.plugged_spiral(H, W, cls)[None]]
    return np.concatenate(fr)


_CACHE = {}


def _case(F, H, W, conn, cls, area):
    """(frames, target, reference out, reference info) -- computed once per case and shared, never modified."""
    key = (F, H, W, conn, cls, area)
    if key not in _CACHE:
        frames = _frames(F, H, W, cls)
        tr = np.random.default_rng(H * 7 + W)
        target = np.roll(frames, (1, 2), (1, 2))                 # overlaps the mask's blobs in part
        target[tr.random(target.shape) < 0.3] = cls              # ... and its holes
        target[-1] = 255                                         # an unlabelled frame
        _CACHE[key] = (frames, target) + Hr.fill_holes_frames(frames, cls, conn, area, target)
    return _CACHE[key]


def test_the_shapes_lie_on_both_sides_of_the_split(hip):
    need = hip.load().gdkvm_fill_holes_workspace_bytes
    assert need(*LAST_LDS) == 0 and need(6, 112, 112) == 0
    assert need(*FIRST_WS) == 2 * ((121 * 127 + 3) // 4 * 4) * 4 and need(2, 256, 256) == 2 * 65536 * 4
    assert LAST_LDS[1] * LAST_LDS[2] == 15360 and FIRST_WS[1] * FIRST_WS[2] == 15367     # the last pixel count with the labels in LDS, and 7 more


@pytest.mark.parametrize("F,H,W", SHAPES)
def test_fill_holes_matches_the_reference(hip, F, H, W):
    for conn, cls, area in _combos(H, W):
        frames, target, want_out, want_info = _case(F, H, W, conn, cls, area)
        if (conn, cls, area) == (4, 1, 4) and H >= 13 and W >= 13:
            # no case is vacuous: some hole is filled and some hole is left open
            assert want_info[:, 1].sum() > 0 and (want_info[:, 0] - want_info[:, 1]).sum() > 0 and want_info[:, 6].sum() > 0
        dm, dt = torch.from_numpy(frames).cuda(), torch.from_numpy(target).cuda()
        out, info = hip.fill_holes(dm, cls=cls, connectivity=conn, max_area=area, target=dt)
        assert out.shape == dm.shape and out.dtype == torch.uint8 and info.shape == (frames.shape[0], 8) and info.dtype == torch.int32
        got_info = info.cpu().numpy()
        assert np.array_equal(got_info, want_info), (conn, cls, area, np.flatnonzero((got_info != want_info).any(1)))
        assert np.array_equal(out.cpu().numpy(), want_out), (conn, cls, area)
        assert torch.equal(dm.cpu(), torch.from_numpy(frames))                               # the input is left alone
        # without a target: the same mask, fields 5..7 are zero
        out2, info2 = hip.fill_holes(dm, cls=cls, connectivity=conn, max_area=area)
        assert torch.equal(out2, out) and torch.equal(info2[:, :5], info[:, :5]) and not info2[:, 5:].any()
        # in place equals out of place
        work = dm.clone()
        out3, info3 = hip.fill_holes(work, cls=cls, connectivity=conn, max_area=area, target=dt, out=work)
        assert out3 is work and torch.equal(work, out) and torch.equal(info3, info)
        # the class's counts of the filled mask, exactly
        o, t = out == cls, dt == cls
        assert torch.equal(hip.class_counts_after_fill(info), torch.stack([(o & t).sum((1, 2)), o.sum((1, 2)), t.sum((1, 2))], -1))
        # idempotent when every hole is filled
        if area == 0:
            again, info4 = hip.fill_holes(out, cls=cls, connectivity=conn)
            assert torch.equal(again, out) and not info4[:, [0, 1, 3, 4]].any()


@pytest.mark.parametrize("F,H,W,offs", [(4, 30, 58, (1, 7, 15)), (2, 121, 127, (1, 15)), (6, 112, 112, (7,))])
def test_fill_holes_at_any_byte_address(hip, F, H, W, offs):
    """mask, target and out as views at odd offsets into buffers: the bytes around the mask are of the class and may neither count nor close a
    hole, the bytes around out keep their sentinel.  out is tried at the mask's own alignment (vector stores) and at another (byte stores)."""
    conn, cls, area = 8, 1, 4
    frames, target, want_out, want_info = _case(F, H, W, conn, cls, area)
    n = frames.size
    for off in offs:
        for out_off in (off, (off + 5) % 16):
            buf = torch.full((n + 48,), cls, dtype=torch.uint8, device="cuda")
            tbuf = torch.full((n + 48,), cls, dtype=torch.uint8, device="cuda")
            obuf = torch.full((n + 48,), 0xEE, dtype=torch.uint8, device="cuda")
            view = buf[off:off + n].view(frames.shape)
            tview = tbuf[16 - off:16 - off + n].view(frames.shape)
            oview = obuf[out_off:out_off + n].view(frames.shape)
            view.copy_(torch.from_numpy(frames)); tview.copy_(torch.from_numpy(target))
            assert view.data_ptr() % 16 == off and oview.data_ptr() % 16 == out_off
            out, info = hip.fill_holes(view, cls=cls, connectivity=conn, max_area=area, target=tview, out=oview)
            assert np.array_equal(info.cpu().numpy(), want_info), (off, out_off)
            assert np.array_equal(oview.cpu().numpy(), want_out), (off, out_off)
            assert (obuf[:out_off] == 0xEE).all() and (obuf[out_off + n:] == 0xEE).all()
            assert (buf[:off] == cls).all() and (buf[off + n:] == cls).all()
        _, info = hip.fill_holes(view, cls=cls, connectivity=conn, max_area=area, target=tview, out=view)      # in place at the odd address
        assert np.array_equal(view.cpu().numpy(), want_out) and np.array_equal(info.cpu().numpy(), want_info)
        assert (buf[:off] == cls).all() and (buf[off + n:] == cls).all()


@pytest.mark.parametrize("H,W", [(112, 112), (144, 160)])
def test_fill_holes_is_reproducible_and_capturable(hip, H, W):
    """LDS form and workspace form: two calls agree; a captured call replays on new input (the workspace belongs to the graph's pool)."""
    a, b = _frames(2, H, W, 1)[[0, 1, 2, 4, -3, -1]], _frames(2, H, W, 1)[[1, 0, 3, 5, -2, -1]]
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    first, second = hip.fill_holes(da, target=db), hip.fill_holes(da, target=db)
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    static, static_t = da.clone(), db.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = hip.fill_holes(static, cls=1, connectivity=4, max_area=0, target=static_t)
    static.copy_(db); static_t.copy_(da)
    g.replay()
    torch.cuda.synchronize()
    want = hip.fill_holes(db, cls=1, connectivity=4, max_area=0, target=da)
    assert all(torch.equal(x, y) for x, y in zip(out, want))
    ref_out, ref_info = Hr.fill_holes_frames(b, 1, 4, 0, a)
    assert ref_info[:, 1].sum() > 0
    assert np.array_equal(out[0].cpu().numpy(), ref_out) and np.array_equal(out[1].cpu().numpy(), ref_info)


def test_lv_measure_of_the_cleaned_mask_is_the_clean_measurement(hip):
    """The feature's purpose, on the device: ellipse + island + punched holes -> largest_component -> fill_holes equals the clean ellipse, and
    lv_measure / lv_ef of it equal the clean ones on every output."""
    clean = np.stack([R.ellipse_mask(112, 112, 56, 56, 40, 18, 20), R.ellipse_mask(112, 112, 56, 56, 32, 13, 20),
                      R.ellipse_mask(112, 112, 50, 60, 36, 15, 150), R.ellipse_mask(112, 112, 56, 56, 40, 18, 20)])
    dirty = clean.copy()
    for f, (cy, cx, r) in enumerate(((12, 12, 4), (12, 100, 6), (100, 15, 8), (100, 100, 5))):
        C.disc(dirty[f], cy, cx, r)                                                          # an island ...
        C.disc(dirty[f], cy, cx, 1, value=0)                                                 # ... with a hole of its own
    for f, (cy, cx, r, v) in enumerate(((56, 56, 4, 0), (56, 56, 6, 2), (50, 60, 3, 255), (70, 61, 5, 3))):
        C.disc(dirty[f], cy, cx, r, value=v)
        assert (clean[f][dirty[f] == v] == 1).sum() > 0
    dc, dd = torch.from_numpy(clean).cuda(), torch.from_numpy(dirty).cuda()
    want = hip.lv_measure(dc)
    assert not torch.equal(hip.lv_measure(hip.largest_component(dd)[0])[2][:, 1], want[2][:, 1])     # the holes do move the volume
    ef = lambda m: hip.lv_ef(m[2][..., 1].reshape(2, 2).contiguous(), m[0][..., 0].reshape(2, 2).contiguous())
    for conn in (4, 8):
        kept, _ = hip.largest_component(dd, connectivity=conn)
        out, info = hip.fill_holes(kept, connectivity=4 if conn == 8 else 8, target=dc)
        assert torch.equal(out, dc) and info[:, 0].tolist() == [1] * 4 and info[:, 1].tolist() == [1] * 4
        assert torch.equal(hip.class_counts_after_fill(info), want[0][:, :1].expand(4, 3))   # Dice 1 against the clean target
        got = hip.lv_measure(out)
        assert all(torch.equal(x, y) for x, y in zip(got, want))
        assert all(torch.equal(x, y) for x, y in zip(ef(got), ef(want)))


def test_leading_dimensions_are_kept(hip):
    frames = _frames(2, 30, 58, 2)[:6]
    dm = torch.from_numpy(frames).cuda()
    flat_out, flat_info = hip.fill_holes(dm, cls=2, connectivity=8, max_area=9, target=dm)
    out, info = hip.fill_holes(dm.view(2, 3, 30, 58), cls=2, connectivity=8, max_area=9, target=dm.view(2, 3, 30, 58))
    assert out.shape == (2, 3, 30, 58) and info.shape == (2, 3, 8)
    assert torch.equal(out.view(6, 30, 58), flat_out) and torch.equal(info.view(6, 8), flat_info)
    one, one_info = hip.fill_holes(dm[0], cls=2, connectivity=8, max_area=9, target=dm[0])
    assert one.shape == (30, 58) and one_info.shape == (8,) and torch.equal(one, flat_out[0]) and torch.equal(one_info, flat_info[0])
    assert hip.class_counts_after_fill(info).shape == (2, 3, 3)


def test_eval_reports_the_fill_holes_block_and_changes_nothing_else(hip, tmp_path):
    """eval.py on the tiny synthetic split (32 clips of 4 frames, every frame labelled, seeded random weights) with the key on and with it
    off: the block is there with its keys in order, and every key other than `fill_holes` and `lv` is unchanged."""
    common = ["data.size=64", "data.frames=4", "batch_size=4", f"run_dir={tmp_path}"]

    def run(extra):
        ev = subprocess.run([sys.executable, os.path.join(ROOT, "eval.py")] + common + extra, capture_output=True, text=True, timeout=600)
        assert ev.returncode == 0, ev.stderr[-2000:]
        return json.loads(ev.stdout.strip().splitlines()[-1])

    on, off = run(["data.lv_fill_holes=4"]), run([])
    assert "fill_holes" not in off
    fh = on["fill_holes"]
    assert list(fh) == ["connectivity", "max_area", "frames_changed", "holes", "pixels_filled", "dice_lv", "iou_lv"]
    assert fh["connectivity"] == 4 and fh["max_area"] == 0 and 0 <= fh["frames_changed"] <= min(fh["holes"], on["clips"] * 4)
    assert fh["pixels_filled"] >= fh["holes"] >= 0 and 0 <= fh["iou_lv"] <= fh["dice_lv"] <= 1
    if fh["pixels_filled"] == 0:
        assert fh["dice_lv"] == on["dice_per_class"][1] and fh["iou_lv"] == on["iou_per_class"][1] and on["lv"] == off["lv"]
    assert {k: v for k, v in on.items() if k not in ("fill_holes", "lv")} == {k: v for k, v in off.items() if k != "lv"}
