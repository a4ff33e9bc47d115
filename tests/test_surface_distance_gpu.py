"""gdkvm_surface_distance on the device against tests/surface_reference.py, bit for bit: all eight integers of every frame.  The shapes sit where
the kernel can go wrong rather than at the workload's size: both sides of the LDS / workspace split (14336 pixels), frames whose H*W is no
multiple of 16 (every frame after the first starts unaligned) or of 32 (bitmap words shared by two rows), one-pixel-wide frames, one long row
per 64 lanes."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import cc_reference as C
from tests import lv_reference as R
from tests import surface_reference as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (frames of the random recipe, H, W): the cfg2 mask; exactly the last LDS size and the first workspace size; two larger workspace sizes; H*W =
# 1740 and 195 (unaligned frames with heads and tails); one long row per 64 lanes; single rows / columns; one pixel
SHAPES = [(6, 112, 112), (2, 112, 128), (2, 113, 127), (2, 256, 256), (2, 320, 272), (4, 30, 58), (5, 15, 13), (2, 8, 1024), (3, 1, 37),
          (3, 37, 1), (1, 1, 1)]

_CACHE = {}


def _case(F, H, W, cls):
    """(mask, target, reference records) -- computed once per case and shared, never modified."""
    key = (F, H, W, cls)
    if key not in _CACHE:
        mask, target = S.case_frames(F, H, W, cls)
        _CACHE[key] = (mask, target, S.surface_distance_frames(mask, target, cls))
    return _CACHE[key]


def _check(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want), (what, [(int(f), got[f].tolist(), want[f].tolist()) for f in np.flatnonzero((got != want).any(1))[:4]])


@pytest.mark.parametrize("F,H,W", SHAPES)
def test_surface_distance_matches_the_reference(hip, F, H, W):
    for cls in (1, 2):
        mask, target, want = _case(F, H, W, cls)
        dm, dt = torch.from_numpy(mask).cuda(), torch.from_numpy(target).cuda()
        surf = hip.surface_distance(dm, dt, cls=cls)
        assert surf.shape == (mask.shape[0], 8) and surf.dtype == torch.int64
        _check(surf, want, cls)
        assert torch.equal(dm.cpu(), torch.from_numpy(mask)) and torch.equal(dt.cpu(), torch.from_numpy(target))      # the inputs are left alone
        # the directions swap with the arguments; the pooled ranks do not care
        _check(hip.surface_distance(dt, dm, cls=cls), want[:, [1, 0, 3, 2, 5, 4, 6, 7]], (cls, "swapped"))
    if H > 1 and W > 1:                                          # (the random recipe puts both classes into every frame that has room)
        assert (_case(F, H, W, 1)[2][:F, :2] > 0).all()


def test_the_largest_distance_and_the_width_of_the_sums(hip):
    """1024 x 1024: opposite corners give the largest d2 there is (2 * 1023^2 < 2^21); a full-height line against the far column gives 1024
    terms of 1023 * 65536 per direction (a sum just below 2^36)."""
    m, t = np.zeros((2, 1024, 1024), np.uint8), np.zeros((2, 1024, 1024), np.uint8)
    m[0, 0, 0] = 1; t[0, 1023, 1023] = 1
    m[1, :, 0] = 1; t[1, :, 1023] = 1
    d2 = 2 * 1023 * 1023
    r = math.isqrt(d2 << 32)
    want = np.asarray([[1, 1, d2, d2, r, r, d2, d2], [1024, 1024, 1023 ** 2, 1023 ** 2, 1024 * 1023 * 65536, 1024 * 1023 * 65536, 1023 ** 2, 1023 ** 2]],
                      np.int64)
    _check(hip.surface_distance(torch.from_numpy(m).cuda(), torch.from_numpy(t).cuda()), want, "1024")


@pytest.mark.parametrize("F,H,W,offs", [(4, 30, 58, (1, 7, 15)), (2, 113, 127, (1, 15)), (6, 112, 112, (7,))])
def test_surface_distance_at_any_byte_address(hip, F, H, W, offs):
    """mask and target as views at odd offsets into buffers filled with the class: the bytes around them may neither count nor shield a
    border pixel from being surface."""
    cls = 1
    mask, target, want = _case(F, H, W, cls)
    n = mask.size
    for off in offs:
        buf = torch.full((n + 48,), cls, dtype=torch.uint8, device="cuda")
        tbuf = torch.full((n + 48,), cls, dtype=torch.uint8, device="cuda")
        view = buf[off:off + n].view(mask.shape)
        tview = tbuf[16 - off:16 - off + n].view(mask.shape)
        view.copy_(torch.from_numpy(mask)); tview.copy_(torch.from_numpy(target))
        assert view.data_ptr() % 16 == off and tview.data_ptr() % 16 == 16 - off
        _check(hip.surface_distance(view, tview, cls=cls), want, off)
        assert (buf[:off] == cls).all() and (buf[off + n:] == cls).all() and (tbuf[:16 - off] == cls).all()


@pytest.mark.parametrize("H,W", [(112, 112), (144, 160)])
def test_surface_distance_is_reproducible_and_capturable(hip, H, W):
    """LDS form and workspace form: two calls agree; a captured call replays on new input (the workspace belongs to the graph's pool)."""
    a, ta = S.case_frames(3, H, W, 1)
    b, tb = S.random_frames(a.shape[0], H, W, seed=12), S.random_frames(a.shape[0], H, W, seed=13)
    da, dta, db, dtb = (torch.from_numpy(x).cuda() for x in (a, ta, b, tb))
    assert torch.equal(hip.surface_distance(da, dta), hip.surface_distance(da, dta))
    static, static_t = da.clone(), dta.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = hip.surface_distance(static, static_t, cls=1)
    static.copy_(db); static_t.copy_(dtb)
    g.replay()
    torch.cuda.synchronize()
    _check(out, S.surface_distance_frames(b, tb, 1), "replay")
    assert torch.equal(out, hip.surface_distance(db, dtb))


def test_leading_dimensions_are_kept_and_the_metrics_follow(hip):
    mask, target, want = _case(4, 30, 58, 2)
    F = mask.shape[0] // 2 * 2
    dm, dt = torch.from_numpy(mask[:F]).cuda(), torch.from_numpy(target[:F]).cuda()
    flat = hip.surface_distance(dm, dt, cls=2)
    surf = hip.surface_distance(dm.view(2, F // 2, 30, 58), dt.view(2, F // 2, 30, 58), cls=2)
    assert surf.shape == (2, F // 2, 8) and torch.equal(surf.view(F, 8), flat)
    one = hip.surface_distance(dm[0], dt[0], cls=2)
    assert one.shape == (8,) and torch.equal(one, flat[0])
    met, valid = hip.surface_metrics(surf)                       # on the device, from the device's record
    assert met.is_cuda and met.shape == (2, F // 2, 3) and valid.shape == (2, F // 2)
    ref = [S.metrics_ref(r) for r in want[:F]]
    assert valid.view(F).tolist() == [r[3] for r in ref]
    for got, r in zip(met.view(F, 3).tolist(), ref):
        assert got == pytest.approx(list(r[:3]), rel=1e-14, abs=0)


def test_hd95_after_the_filter_is_the_clean_masks(hip):
    """The purpose: ellipse + far island against the clean ellipse -- HD95 after largest_component equals HD95 of the clean mask and is smaller
    than before."""
    clean = np.stack([R.ellipse_mask(112, 112, 56, 56, 40, 18, 20), R.ellipse_mask(112, 112, 56, 56, 32, 13, 20),
                      R.ellipse_mask(112, 112, 50, 60, 36, 15, 150)])
    target = np.stack([R.ellipse_mask(112, 112, 57, 54, 38, 19, 24), R.ellipse_mask(112, 112, 55, 57, 33, 12, 17),
                       R.ellipse_mask(112, 112, 52, 59, 35, 16, 146)])
    dirty = clean.copy()
    for f, (cy, cx, r) in enumerate(((12, 12, 5), (12, 100, 6), (100, 15, 8))):
        C.disc(dirty[f], cy, cx, r)
    dc, dd, dt = (torch.from_numpy(x).cuda() for x in (clean, dirty, target))
    want = hip.surface_distance(dc, dt)
    before = hip.surface_distance(dd, dt)
    filtered, info = hip.largest_component(dd, cls=1, connectivity=4, fill=0, target=dt)
    after = hip.surface_distance(filtered, dt)
    assert torch.equal(filtered, dc) and torch.equal(after, want)
    _check(want, S.surface_distance_frames(clean, target, 1), "clean")
    _check(before, S.surface_distance_frames(dirty, target, 1), "dirty")
    m_want, m_before, m_after = (hip.surface_metrics(s)[0] for s in (want, before, after))
    assert torch.equal(m_after, m_want)
    assert (m_after[:, 1] < m_before[:, 1]).all() and (m_after[:, 0] < m_before[:, 0]).all() and (m_after[:, 2] < m_before[:, 2]).all()


def test_eval_reports_the_surface_block_and_changes_nothing_else(hip, tmp_path):
    """eval.py on the tiny synthetic split (32 clips of 4 frames, every frame labelled, seeded random weights) with the key on and with it
    off: the surface block is there, its means are ordered, every labelled frame is counted once, and every other key is unchanged."""
    common = ["data.size=64", "data.frames=4", "batch_size=4", f"run_dir={tmp_path}"]

    def run(extra):
        ev = subprocess.run([sys.executable, os.path.join(ROOT, "eval.py")] + common + extra, capture_output=True, text=True, timeout=600)
        assert ev.returncode == 0, ev.stderr[-2000:]
        return json.loads(ev.stdout.strip().splitlines()[-1])

    on, off = run(["data.surface_class=1"]), run([])
    assert "surface" not in off
    sf = on["surface"]
    assert list(sf) == ["class", "frames", "frames_one_empty", "hd_mean", "hd95_mean", "assd_mean"] and sf["class"] == 1
    assert 0 < sf["assd_mean"] <= sf["hd95_mean"] <= sf["hd_mean"] <= math.sqrt(2) * 63
    # the synthetic target has class 1 in every frame, so a frame either has both surfaces or lacks the prediction's: together all 128 frames
    assert sf["frames"] > 0 and sf["frames"] + sf["frames_one_empty"] == on["clips"] * 4
    assert {k: v for k, v in on.items() if k != "surface"} == off
