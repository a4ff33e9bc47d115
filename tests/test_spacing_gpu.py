"""gdkvm_surface_distance_mm and gdkvm_lv_measure_mm on the device against tests/spacing_reference.py: every integer bit for bit (the LV axis
within one unit, everything behind it against the reference evaluated with the device's own axis), fp64 outputs to 1e-12.  The shapes sit
where the kernels can go wrong: the cfg2 mask in the LDS form, exactly the LDS form's capacity and one row above it, frames whose H W is no
multiple of 16 or 32, one-pixel-wide frames, one long row per 64 lanes, the largest squared distance 45 bits hold; for the LV kernel both of
its forms (match bits in registers up to 256 x 256, vectors read again above)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import spacing_reference as P
from tests import surface_reference as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = P.Q
LDS_PIX = 18432                                                  # GDKVM_SURFACE_MM_LDS_PIXELS = 144 * 128
# (frames of the random recipe, H, W)
SURFACE_SHAPES = [(6, 112, 112), (2, 113, 127), (4, 30, 58), (3, 1, 37), (3, 37, 1), (2, 8, 1024), (1, 144, 128), (1, 145, 128)]
SURFACE_SPACINGS = [(330, 468), (1, 4095)]

_CACHE = {}


def _case(F, H, W):
    """(mask, target) of class 1 -- built once per shape and shared, never modified."""
    if (F, H, W) not in _CACHE:
        _CACHE[(F, H, W)] = S.case_frames(F, H, W, 1)
    return _CACHE[(F, H, W)]


def _want(F, H, W, ry, rx):
    key = (F, H, W, ry, rx)
    if key not in _CACHE:
        _CACHE[key] = P.surface_distance_mm_frames(*_case(F, H, W), (ry, rx), 1)
    return _CACHE[key]


def _check(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want), (what, [(int(f), got[f].tolist(), want[f].tolist()) for f in np.flatnonzero((got != want).any(1))[:4]])


def _sp(*pairs):
    return torch.tensor(pairs, dtype=torch.int32)


def test_the_header_and_ops_agree_on_the_lds_capacity(hip):
    assert hip.SURFACE_MM_LDS_PIXELS == LDS_PIX and hip.SPACING_UM_MAX == P.UM_MAX
    assert hip._bytes("gdkvm_surface_distance_mm_workspace_bytes", None, 3, 144, 128) == 0
    per_frame = (8 * 145 * 128 + 16 * (((145 * 128 + 31) // 32 + 3) // 4 * 4) + 127) // 128 * 128
    assert hip._bytes("gdkvm_surface_distance_mm_workspace_bytes", None, 3, 145, 128) == 3 * per_frame


@pytest.mark.parametrize("ry,rx", SURFACE_SPACINGS)
@pytest.mark.parametrize("F,H,W", SURFACE_SHAPES)
def test_surface_distance_mm_matches_the_reference(hip, F, H, W, ry, rx):
    mask, target = _case(F, H, W)
    want = _want(F, H, W, ry, rx)
    dm, dt = torch.from_numpy(mask).cuda(), torch.from_numpy(target).cuda()
    surf = hip.surface_distance_mm(dm, dt, _sp((ry, rx)), cls=1)
    assert surf.shape == (mask.shape[0], 8) and surf.dtype == torch.int64
    _check(surf, want, (ry, rx))
    assert torch.equal(dm.cpu(), torch.from_numpy(mask)) and torch.equal(dt.cpu(), torch.from_numpy(target))      # the inputs are left alone
    _check(hip.surface_distance_mm(dt, dm, _sp((ry, rx)).cuda(), cls=1), want[:, [1, 0, 3, 2, 5, 4, 6, 7]], "swapped, device spacing")
    if H > 1 and W > 1:
        assert (want[:F, :2] > 0).all()


def test_every_clip_takes_its_own_spacing_and_a_bad_one_is_marked(hip):
    """[B, T, H, W] against [B, 1, 2]: four clips, four spacings; then per-frame spacings of which one is 0 and one 4096 (a device tensor:
    a host tensor with them is refused before anything is launched)."""
    mask, target = _case(4, 30, 58)
    B, T = 4, mask.shape[0] // 4
    m, t = mask[:B * T], target[:B * T]
    clip_sp = [(330, 468), (1, 4095), (4095, 1), (3, 7)]
    dm, dt = torch.from_numpy(m).cuda().view(B, T, 30, 58), torch.from_numpy(t).cuda().view(B, T, 30, 58)
    surf = hip.surface_distance_mm(dm, dt, _sp(*clip_sp).view(B, 1, 2))
    assert surf.shape == (B, T, 8)
    frame_sp = [clip_sp[f // T] for f in range(B * T)]
    _check(surf.view(B * T, 8), P.surface_distance_mm_frames(m, t, frame_sp, 1), "per clip")
    frame_sp[1], frame_sp[B * T - 2] = (0, 468), (330, 4096)
    dev_sp = _sp(*frame_sp).cuda().view(B, T, 2)
    surf = hip.surface_distance_mm(dm, dt, dev_sp)
    want = P.surface_distance_mm_frames(m, t, frame_sp, 1)
    assert want[1].tolist() == [-1] * 8 and want[B * T - 2].tolist() == [-1] * 8
    _check(surf.view(B * T, 8), want, "per frame")
    met, valid = hip.surface_metrics_mm(surf)
    assert not valid.view(-1)[1] and not valid.view(-1)[B * T - 2] and not met.view(-1, 3)[1].any() and valid.view(-1)[0]
    for bad in ((0, 468), (330, 4096), (-1, 5)):
        with pytest.raises(hip.GdkvmError, match="spacing_um"):
            hip.surface_distance_mm(dm, dt, _sp(bad))
    for bad in (torch.tensor([[330.0, 468.0]]), _sp((330, 468)).long(), torch.tensor([330, 468, 1], dtype=torch.int32), _sp(*clip_sp[:3]).view(3, 1, 2)):
        with pytest.raises(hip.GdkvmError, match="spacing_um"):
            hip.surface_distance_mm(dm, dt, bad)


def test_the_width_of_the_words(hip):
    """1024 x 1024 at 4095 x 4095 um: single pixels in opposite corners give the largest d2 there is, 2 (1023 * 4095)^2 < 2^45, a root below
    2^31 in the sums; a full-height line against the far column gives 1024 terms of 1023 * 4095 * 256 per direction."""
    m, t = np.zeros((2, 1024, 1024), np.uint8), np.zeros((2, 1024, 1024), np.uint8)
    m[0, 0, 0] = 1; t[0, 1023, 1023] = 1
    m[1, :, 0] = 1; t[1, :, 1023] = 1
    d2 = 2 * (1023 * 4095) ** 2
    assert 1 << 44 < d2 < 1 << 45
    r = math.isqrt(d2 << 16)
    line = (1023 * 4095) ** 2
    want = np.asarray([[1, 1, d2, d2, r, r, d2, d2], [1024, 1024, line, line, 1024 * 1023 * 4095 * 256, 1024 * 1023 * 4095 * 256, line, line]], np.int64)
    surf = hip.surface_distance_mm(torch.from_numpy(m).cuda(), torch.from_numpy(t).cuda(), _sp((4095, 4095)))
    _check(surf, want, "1024")
    met, valid = hip.surface_metrics_mm(surf)
    assert valid.all() and met[0, 0].item() == pytest.approx(math.sqrt(2) * 1023 * 4.095, rel=1e-14)


def test_unit_spacing_gives_the_pixel_kernels_integers(hip):
    for F, H, W in ((6, 112, 112), (1, 145, 128), (4, 30, 58)):
        mask, target = _case(F, H, W)
        dm, dt = torch.from_numpy(mask).cuda(), torch.from_numpy(target).cuda()
        pix, one = hip.surface_distance(dm, dt), hip.surface_distance_mm(dm, dt, _sp((1, 1)))
        cols = [0, 1, 2, 3, 6, 7]
        assert torch.equal(pix[:, cols], one[:, cols])


def test_surface_metrics_mm_are_the_float_formulas(hip):
    mask, target = _case(4, 30, 58)
    F = mask.shape[0] // 2 * 2
    want = _want(4, 30, 58, 330, 468)[:F]
    surf = hip.surface_distance_mm(torch.from_numpy(mask[:F]).cuda().view(2, F // 2, 30, 58), torch.from_numpy(target[:F]).cuda().view(2, F // 2, 30, 58),
                                   _sp((330, 468)))
    assert surf.shape == (2, F // 2, 8)
    met, valid = hip.surface_metrics_mm(surf)
    assert met.is_cuda and met.dtype == torch.float64 and met.shape == (2, F // 2, 3) and valid.shape == (2, F // 2)
    ref = [P.metrics_mm_ref(r) for r in want]
    assert valid.view(F).tolist() == [r[3] for r in ref] and not all(r[3] for r in ref) and any(r[3] for r in ref)
    for got, r in zip(met.view(F, 3).tolist(), ref):
        assert got == pytest.approx(list(r[:3]), rel=1e-14, abs=0)
    host, host_valid = hip.surface_metrics_mm(torch.from_numpy(want))            # pure torch on either device
    assert torch.allclose(host, met.view(F, 3).cpu(), rtol=1e-14, atol=0.0) and torch.equal(host_valid, valid.view(F).cpu())
    # the summary and the statistics serve unchanged
    sums = hip.surface_summary(met, valid, surf, torch.ones_like(valid))
    st = hip.surface_stats(sums.cpu())
    assert st["frames"] == sum(r[3] for r in ref) and st["hd_mean"] == pytest.approx(sum(r[0] for r in ref) / st["frames"], rel=1e-13)


@pytest.mark.parametrize("F,H,W,offs", [(4, 30, 58, (1, 7, 15)), (2, 113, 127, (15,)), (1, 145, 128, (7,))])
def test_surface_distance_mm_at_any_byte_address(hip, F, H, W, offs):
    mask, target = _case(F, H, W)
    want = _want(F, H, W, 330, 468)
    n = mask.size
    for off in offs:
        buf = torch.full((n + 48,), 1, dtype=torch.uint8, device="cuda")
        tbuf = torch.full((n + 48,), 1, dtype=torch.uint8, device="cuda")
        view = buf[off:off + n].view(mask.shape)
        tview = tbuf[16 - off:16 - off + n].view(mask.shape)
        view.copy_(torch.from_numpy(mask)); tview.copy_(torch.from_numpy(target))
        assert view.data_ptr() % 16 == off and tview.data_ptr() % 16 == 16 - off
        _check(hip.surface_distance_mm(view, tview, _sp((330, 468))), want, off)
        assert (buf[:off] == 1).all() and (buf[off + n:] == 1).all() and (tbuf[:16 - off] == 1).all()


@pytest.mark.parametrize("H,W", [(112, 112), (145, 128)])
def test_surface_distance_mm_is_reproducible_and_capturable(hip, H, W):
    """LDS form and workspace form: two calls agree; a captured call (one stream) replays on new masks and new spacings."""
    a, ta = _case(6 if H == 112 else 1, H, W)
    b, tb = S.random_frames(a.shape[0], H, W, seed=12), S.random_frames(a.shape[0], H, W, seed=13)
    da, dta, db, dtb = (torch.from_numpy(x).cuda() for x in (a, ta, b, tb))
    sp_a, sp_b = _sp((330, 468)).cuda().expand(a.shape[0], 2).contiguous(), _sp((468, 330)).cuda().expand(a.shape[0], 2).contiguous()
    first = hip.surface_distance_mm(da, dta, sp_a)
    assert torch.equal(first, hip.surface_distance_mm(da, dta, sp_a))
    static, static_t, static_sp = da.clone(), dta.clone(), sp_a.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = hip.surface_distance_mm(static, static_t, static_sp)
    static.copy_(db); static_t.copy_(dtb); static_sp.copy_(sp_b)
    g.replay()
    torch.cuda.synchronize()
    _check(out, P.surface_distance_mm_frames(b, tb, (468, 330), 1), "replay")
    assert torch.equal(out, hip.surface_distance_mm(db, dtb, sp_b))


# ---- gdkvm_lv_measure_mm ---------------------------------------------------------------------------------------------------------------------------
LV_SHAPES = [(3, 112, 112), (2, 113, 127), (2, 256, 256), (3, 30, 58), (2, 320, 272)]       # the last: the form that reads its vectors again
LV_SPACINGS = [(330, 468), (468, 330), (300, 300), (1, 4095)]


def _lv_check(ops, frames_np, frames_dev, spacing, cls, D):
    """spacing: one pair per frame.  Returns the device's (stats, disks, geom) as numpy."""
    F = frames_np.shape[0]
    stats, disks, geom = ops.lv_measure_mm(frames_dev, _sp(*spacing), cls=cls, disks=D)
    assert stats.shape == (F, 12) and stats.dtype == torch.int64 and disks.shape == (F, D) and disks.dtype == torch.int64
    assert geom.shape == (F, 6) and geom.dtype == torch.float64
    stats, disks, geom = stats.cpu().numpy(), disks.cpu().numpy(), geom.cpu().numpy()
    for f in range(F):
        ry, rx = spacing[f]
        ref = P.lv_measure_mm_ref(frames_np[f], ry, rx, cls, D)
        assert stats[f, :6].tolist() == ref["stats"][:6], (f, cls, D)
        if ref["stats"][0] == 0:
            assert not stats[f].any() and not disks[f].any() and not geom[f].any()
            continue
        for i in (6, 7, 11):                                     # Vx, Vy, E: a moved rint tie at most
            assert abs(int(stats[f, i]) - ref["stats"][i]) <= 1, (f, i, stats[f].tolist(), ref["stats"])
        # k: a few fp64 roundings apart; a structural error (a wrong gcd, a swapped px / py) is off by 2^-17 or more
        assert abs(geom[f, 4] - ref["geom"][4]) <= 1e-12 * ref["geom"][4], (f, geom[f, 4], ref["geom"][4])
        own = P.lv_measure_mm_ref(frames_np[f], ry, rx, cls, D, axis=(int(stats[f, 6]), int(stats[f, 7]), int(stats[f, 11]), float(geom[f, 4])))
        assert stats[f].tolist() == own["stats"], (f, cls, D)
        assert disks[f].tolist() == own["disks"], (f, cls, D)
        assert int(disks[f].sum()) == int(stats[f, 0]) ** 2 * D * int(stats[f, 11])
        assert np.allclose(geom[f], own["geom"], rtol=1e-12, atol=0.0), (f, cls, D, geom[f], own["geom"])
    return stats, disks, geom


@pytest.mark.parametrize("F,H,W", LV_SHAPES)
def test_lv_measure_mm_matches_the_reference(hip, F, H, W):
    frames = S.random_frames(F, H, W, seed=H * 1000 + W)
    dev = torch.from_numpy(frames).cuda()
    for ry, rx in LV_SPACINGS if H * W <= 256 * 256 else LV_SPACINGS[:1]:
        for cls, D in ((1, 20), (2, 7)) if (ry, rx) == (330, 468) else ((1, 20),):
            stats, disks, _ = _lv_check(hip, frames, dev, [(ry, rx)] * F, cls, D)
            if (ry, rx) == (300, 300):                           # isotropic: the pixel kernel's integers wherever the axes agree
                p_stats, p_disks, p_geom = (x.cpu().numpy() for x in hip.lv_measure(dev, cls=cls, disks=D))
                same = (stats[:, 6:8] == p_stats[:, 6:8]).all(1)
                assert same.any() and (stats[:, 11] == Q).all()
                assert np.array_equal(stats[same, :11], p_stats[same, :11]) and np.array_equal(disks[same], p_disks[same])
                assert (np.abs(stats[:, 6:8] - p_stats[:, 6:8]) <= 1).all() and np.array_equal(stats[:, :6], p_stats[:, :6])


def test_lv_measure_mm_spacing_per_frame_corner_frames_and_leading_dimensions(hip):
    """Each frame its own spacing ([B, 1, 2] against [B, T, H, W]); an empty frame is zeros; a spacing of 0 or 4096 (device tensor) is -1
    everywhere; a host tensor with one is refused."""
    H, W = 41, 35
    fr = S.random_frames(6, H, W, seed=9)
    fr[2] = 0                                                    # empty
    fr[3] = 0; fr[3, 5:7, 9:11] = 1                              # 2 x 2 square: r == 0 in pixels, not in micrometres
    clip_sp = [(330, 468), (468, 330), (1, 4095)]
    frame_sp = [clip_sp[f // 2] for f in range(6)]
    dev = torch.from_numpy(fr).cuda()
    flat = _lv_check(hip, fr, dev, frame_sp, 1, 20)
    assert flat[0][3, 0] == 4 and flat[0][3, 6:8].tolist() == [0, Q]             # rows of 468 um, columns of 330: the square is higher than wide
    s, d, g = hip.lv_measure_mm(dev.view(3, 2, H, W), _sp(*clip_sp).view(3, 1, 2), cls=1, disks=20)
    assert s.shape == (3, 2, 12) and d.shape == (3, 2, 20) and g.shape == (3, 2, 6)
    assert np.array_equal(s.view(6, 12).cpu().numpy(), flat[0]) and np.array_equal(d.view(6, 20).cpu().numpy(), flat[1])
    assert np.array_equal(g.view(6, 6).cpu().numpy(), flat[2])
    frame_sp[0], frame_sp[5] = (0, 468), (330, 4096)
    s, d, g = hip.lv_measure_mm(dev, _sp(*frame_sp).cuda(), cls=1, disks=7)
    for f in (0, 5):
        assert (s[f] == -1).all() and (d[f] == -1).all() and (g[f] == -1.0).all()
    assert np.array_equal(s[1:5, :6].cpu().numpy(), flat[0][1:5, :6]) and not s[2].any()
    with pytest.raises(hip.GdkvmError, match="spacing_um"):
        hip.lv_measure_mm(dev, _sp(*frame_sp))
    # the mL curve goes into lv_ef as it is
    vol, npix = g[1:5, 1].reshape(1, 4).contiguous(), s[1:5, 0].reshape(1, 4).contiguous()
    idx, val = hip.lv_ef(vol, npix)
    v = vol[0].tolist()
    assert idx[0, 2] == 3 and val[0, 0].item() == max(v[0], v[2], v[3]) and val[0, 1].item() == min(v[0], v[2], v[3])


@pytest.mark.parametrize("F,H,W,offs", [(3, 30, 58, (1, 7, 15)), (2, 321, 273, (9,))])
def test_lv_measure_mm_mask_at_any_byte_address(hip, F, H, W, offs):
    frames = S.random_frames(F, H, W, seed=5)
    for off in offs:
        buf = torch.full((F * H * W + 32,), 1, dtype=torch.uint8, device="cuda")             # class bytes around the view: none may count
        view = buf[off:off + F * H * W].view(F, H, W)
        view.copy_(torch.from_numpy(frames))
        assert view.data_ptr() % 16 == off
        _lv_check(hip, frames, view, [(330, 468)] * F, 1, 20)


def test_lv_measure_mm_is_reproducible_and_capturable(hip):
    a, b = S.random_frames(4, 112, 112, seed=11), S.random_frames(4, 112, 112, seed=12)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    sp = _sp((330, 468)).cuda().expand(4, 2).contiguous()
    first, second = hip.lv_measure_mm(da, sp), hip.lv_measure_mm(da, sp)
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    static = da.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = hip.lv_measure_mm(static, sp, cls=1, disks=20)
    static.copy_(db)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(out, hip.lv_measure_mm(db, sp, cls=1, disks=20)))
    _lv_check(hip, b, db, [(330, 468)] * 4, 1, 20)


# ---- eval.py ---------------------------------------------------------------------------------------------------------------------------------------
def test_eval_reports_the_mm_blocks_and_changes_nothing_else(hip, tmp_path):
    """eval.py on the tiny synthetic split (which carries no spacing of its own) with data.spacing_um on and off: the two blocks appear and
    every other key keeps its value.  At 1000 x 1000 um a pixel is a millimetre: the EF statistics in mL are those in pixels, and so are the
    mean HD and HD95; the mean ASSD agrees to 2.6e-5 -- each of its terms is rounded down to 2^-8 um here and to 2^-16 pixel there (at most
    1.53e-5 mm apart), and both means are printed rounded to 1e-5."""
    common = ["data.size=64", "data.frames=4", "batch_size=4", "data.surface_class=1", f"run_dir={tmp_path}"]

    def run(extra):
        ev = subprocess.run([sys.executable, os.path.join(ROOT, "eval.py")] + common + extra, capture_output=True, text=True, timeout=600)
        assert ev.returncode == 0, ev.stderr[-2000:]
        return json.loads(ev.stdout.strip().splitlines()[-1])

    off, on, unit = run([]), run(["data.spacing_um=[330,468]"]), run(["data.spacing_um=[1000,1000]"])
    assert "lv_mm" not in off and "surface_mm" not in off and "lv" in off and "surface" in off
    for res in (on, unit):
        assert {k: v for k, v in res.items() if k not in ("lv_mm", "surface_mm")} == off
        assert list(res["lv_mm"]) == list(off["lv"]) + ["edv_mae_ml", "edv_bias_ml", "esv_mae_ml", "esv_bias_ml"]
        assert list(res["surface_mm"]) == ["frames", "frames_one_empty", "hd_mean_mm", "hd95_mean_mm", "assd_mean_mm"]
        assert res["surface_mm"]["frames"] == off["surface"]["frames"] and res["surface_mm"]["frames_one_empty"] == off["surface"]["frames_one_empty"]
        assert res["lv_mm"]["clips_with_ef"] == off["lv"]["clips_with_ef"] > 0
        assert res["lv_mm"]["edv_mae_ml"] >= abs(res["lv_mm"]["edv_bias_ml"]) and res["lv_mm"]["esv_mae_ml"] >= abs(res["lv_mm"]["esv_bias_ml"])
    sm = on["surface_mm"]
    assert 0 < sm["assd_mean_mm"] <= sm["hd95_mean_mm"] <= sm["hd_mean_mm"] <= math.hypot(63 * 0.330, 63 * 0.468)
    assert 0.330 * off["surface"]["hd_mean"] - 1e-5 <= sm["hd_mean_mm"] <= 0.468 * off["surface"]["hd_mean"] + 1e-5     # (both printed to 1e-5)
    assert {k: unit["lv_mm"][k] for k in off["lv"]} == off["lv"]
    assert unit["surface_mm"]["hd_mean_mm"] == off["surface"]["hd_mean"] and unit["surface_mm"]["hd95_mean_mm"] == off["surface"]["hd95_mean"]
    assert abs(unit["surface_mm"]["assd_mean_mm"] - off["surface"]["assd_mean"]) <= 2.6e-5
