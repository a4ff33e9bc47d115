"""gdkvm_lv_measure / gdkvm_lv_ef on the device against tests/lv_reference.py: integer outputs bit for bit (the axis within one unit of Q, everything
behind it against the reference evaluated with the kernel's own axis), fp64 outputs to 1e-12 (about D + 4 roundings of 2^-53)."""
import numpy as np
import pytest
import torch

from tests import lv_reference as R

pytestmark = pytest.mark.gpu

Q = R.Q
DS, CLASSES = (20, 7, 64), (1, 2)
# (frames, H, W): the cfg2 mask; the largest frame whose match bits stay in registers; beyond it (vectors read again per pass); H*W no multiple
# of 16; H*W = 195 (every frame after the first starts unaligned and has a tail); one long row per 64 lanes
SHAPES = [(6, 112, 112), (3, 256, 256), (2, 320, 272), (4, 30, 58), (5, 15, 13), (2, 8, 1024)]


def _random_frames(F, H, W, seed):
    """Unions of random rotated ellipses of classes 1 and 2, speckle pixels of both elsewhere, a patch of class 3 and one of 255."""
    rng = np.random.default_rng(seed)
    out = np.zeros((F, H, W), np.uint8)
    for f in range(F):
        m = out[f]
        for value in (2, 1, 1):
            la = rng.uniform(0.12, 0.4) * max(H, W)
            sa = rng.uniform(0.08, 0.3) * min(H, W)
            R.ellipse_mask(H, W, rng.uniform(0.3, 0.7) * H, rng.uniform(0.3, 0.7) * W, la, sa, rng.uniform(0, 180), value=value, out=m)
        sp = rng.random((H, W))
        m[sp < 0.004] = 1
        m[sp > 0.996] = 2
        m[: max(H // 8, 1), : max(W // 5, 1)] = 3
        m[H - max(H // 9, 1):, W // 2:] = 255
    return out


def _special_frames(H, W, cls):
    """One frame per corner of the definition."""
    fr = []
    z = lambda: np.zeros((H, W), np.uint8)
    fr.append(z())                                               # empty
    m = z(); m[H // 3, W // 2] = cls; fr.append(m)               # one pixel
    fr.append(np.full((H, W), cls, np.uint8))                    # full frame
    m = z(); m[H // 2, 3:W - 2] = cls; fr.append(m)              # one-row horizontal line
    m = z(); i = np.arange(min(H, W) - 6); m[i + 2, i + 4] = cls; fr.append(m)      # 45-degree diagonal: A == C, B != 0
    m = z(); m[5:7, 9:11] = cls; fr.append(m)                    # 2 x 2 square: r == 0
    m = z(); m[4:9, 7:10] = cls; fr.append(m)                    # shorter than D pixels: a pixel overlaps several disks
    m = z(); m[H - 1, W - 1] = cls; m[0, 0] = cls; fr.append(m)  # first and last byte of the frame
    m = np.full((H, W), 255, np.uint8); m[1:4, 1:3] = cls; m[10, 10] = 3 - cls; fr.append(m)
    return np.stack(fr)


def _check(ops, frames_np, frames_dev, cls, D):
    stats, disks, geom = ops.lv_measure(frames_dev, cls=cls, disks=D)
    F = frames_np.shape[0]
    assert stats.shape == (F, 12) and stats.dtype == torch.int64 and disks.shape == (F, D) and disks.dtype == torch.int64
    assert geom.shape == (F, 4) and geom.dtype == torch.float64
    stats, disks, geom = stats.cpu().numpy(), disks.cpu().numpy(), geom.cpu().numpy()
    for f in range(F):
        ref = R.lv_measure_ref(frames_np[f], cls, D)
        assert stats[f, :6].tolist() == ref["stats"][:6], (f, cls, D)
        assert abs(int(stats[f, 6]) - ref["stats"][6]) <= 1 and abs(int(stats[f, 7]) - ref["stats"][7]) <= 1, (f, stats[f, 6:8], ref["stats"][6:8])
        own = ref if stats[f, 6:8].tolist() == ref["stats"][6:8] else R.lv_measure_ref(frames_np[f], cls, D, axis=(int(stats[f, 6]), int(stats[f, 7])))
        assert stats[f].tolist() == own["stats"], (f, cls, D)
        assert disks[f].tolist() == own["disks"], (f, cls, D)
        assert int(disks[f].sum()) == int(stats[f, 0]) ** 2 * D * Q
        assert np.allclose(geom[f], own["geom"], rtol=1e-12, atol=0.0), (f, cls, D, geom[f], own["geom"])
    return stats, disks, geom


@pytest.mark.parametrize("F,H,W", SHAPES)
def test_lv_measure_matches_the_reference(hip, F, H, W):
    frames = _random_frames(F, H, W, seed=H * 1000 + W)
    dev = torch.from_numpy(frames).cuda()
    for cls in CLASSES:
        for D in DS:
            _check(hip, frames, dev, cls, D)
    # leading dimensions are kept
    if F % 2 == 0:
        s, d, g = hip.lv_measure(dev.view(2, F // 2, H, W), cls=1, disks=7)
        s2, d2, g2 = hip.lv_measure(dev, cls=1, disks=7)
        assert s.shape == (2, F // 2, 12) and d.shape == (2, F // 2, 7) and g.shape == (2, F // 2, 4)
        assert torch.equal(s.view(F, 12), s2) and torch.equal(d.view(F, 7), d2) and torch.equal(g.view(F, 4), g2)


@pytest.mark.parametrize("H,W", [(41, 35), (48, 64)])
def test_lv_measure_corner_frames(hip, H, W):
    for cls in CLASSES:
        frames = _special_frames(H, W, cls)
        dev = torch.from_numpy(frames).cuda()
        for D in DS:
            stats, disks, geom = _check(hip, frames, dev, cls, D)
            assert not stats[0].any() and not disks[0].any() and not geom[0].any()           # empty frame: zeros
            assert stats[1, 0] == 1 and geom[1, 0] == 1.0                                      # one pixel: one pixel long
            assert stats[2, 0] == H * W
            assert stats[3, 6:8].tolist() == [Q, 0] and stats[5, 6:8].tolist() == [0, Q]       # the line's axis; the square's default
            assert stats[4, 6] == stats[4, 7]                                                  # the diagonal


@pytest.mark.parametrize("F,H,W,offs", [(3, 30, 58, (1, 7, 15)), (2, 320, 272, (1,)), (2, 321, 273, (0, 9))])
def test_lv_measure_mask_at_any_byte_address(hip, F, H, W, offs):
    """Head and tail bytes of both kernel forms: the register-resident one and (above 256 x 256) the one that reads its vectors again."""
    frames = _random_frames(F, H, W, seed=5)
    for off in offs:
        buf = torch.full((F * H * W + 32,), 1, dtype=torch.uint8, device="cuda")             # class bytes around the view: none may count
        view = buf[off:off + F * H * W].view(F, H, W)
        view.copy_(torch.from_numpy(frames))
        assert view.data_ptr() % 16 == off
        _check(hip, frames, view, 1, 20)


def test_lv_measure_is_reproducible_and_capturable(hip):
    a = _random_frames(4, 112, 112, seed=11)
    b = _random_frames(4, 112, 112, seed=12)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    first, second = hip.lv_measure(da), hip.lv_measure(da)
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    static = da.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = hip.lv_measure(static, cls=1, disks=20)
        ef = hip.lv_ef(out[2][..., 1].reshape(1, 4), out[0][..., 0].reshape(1, 4))
    static.copy_(db)
    g.replay()
    torch.cuda.synchronize()
    want = hip.lv_measure(db, cls=1, disks=20)
    assert all(torch.equal(x, y) for x, y in zip(out, want))
    want_ef = hip.lv_ef(want[2][..., 1].reshape(1, 4), want[0][..., 0].reshape(1, 4))
    assert all(torch.equal(x, y) for x, y in zip(ef, want_ef))
    _check(hip, b, db, 1, 20)


def _ef_check(ops, vol, npx, pick_vol=None, pick_npix=None, min_pixels=1):
    t = lambda x, dt: None if x is None else torch.from_numpy(np.asarray(x)).to(dt).cuda()
    idx, val = ops.lv_ef(t(vol, torch.float64), t(npx, torch.int64), t(pick_vol, torch.float64), t(pick_npix, torch.int64), min_pixels=min_pixels)
    assert idx.dtype == torch.int32 and val.dtype == torch.float64 and idx.shape == val.shape == (len(vol), 3)
    ridx, rval = R.lv_ef_ref(vol, npx, pick_vol, pick_npix, min_pixels)
    assert idx.cpu().tolist() == ridx
    assert np.allclose(val.cpu().numpy(), np.asarray(rval), rtol=1e-15, atol=0.0)
    return ridx, rval


@pytest.mark.parametrize("T", [10, 70, 200])
def test_lv_ef_matches_the_reference(hip, T):
    rng = np.random.default_rng(T)
    B = 12
    vol = rng.uniform(100.0, 900.0, (B, T))
    npx = rng.integers(0, 40, (B, T))
    npx[npx < 8] = 0                                             # frames without the class
    vol[npx == 0] = 0.0
    for b in range(B):                                           # planted ties of the extremes, highest t first in memory order
        v = np.where(npx[b] >= 5, vol[b], np.nan)
        hi, lo = int(np.nanargmax(v)), int(np.nanargmin(v))
        for k in rng.choice(T, 3, replace=False):
            if npx[b, k] >= 5:
                vol[b, k] = vol[b, hi] if k % 2 else vol[b, lo]
    npx[0] = 0                                                   # no valid frame
    npx[1] = 0; npx[1, T - 1] = 9                                # one
    npx[2] = 0; npx[2, 3] = 9; npx[2, T - 2] = 9                 # two
    vol[2, 3], vol[2, T - 2] = 5.0, 7.0
    vol[3] = 0.0                                                 # EDV == 0
    pick_vol = rng.uniform(1.0, 2.0, (B, T))
    pick_vol[:, 5] = pick_vol[:, 2]
    pick_npix = rng.integers(0, 12, (B, T))
    pick_npix[4] = 0; pick_npix[4, 1] = 7
    for mp in (1, 5, 100):
        ridx, rval = _ef_check(hip, vol, npx, min_pixels=mp)
        assert ridx[0] == [-1, -1, 0]
        if mp <= 5:
            assert ridx[1] == [-1, -1, 1] and ridx[2] == [T - 2, 3, 2] and rval[2] == [7.0, 5.0, 2.0 / 7.0]
            assert ridx[3][2] >= 2 and ridx[3][0] == ridx[3][1] >= 0 and rval[3] == [0.0, 0.0, 0.0]
        _ef_check(hip, vol, npx, pick_vol, pick_npix, min_pixels=mp)


def test_clip_level_ef_on_synthetic_labels(hip):
    """Synthetic clips' own labels as prediction and target: no EF error at all; the target eroded by one pixel has a smaller volume at the
    target's end-diastolic frame."""
    from gdkvm_amd.data import SyntheticEchoClips
    ds = SyntheticEchoClips(16, 10, 64, num_classes=2, as_uint8=True)
    target = torch.stack([ds[i][1] for i in range(16)])
    assert target.shape == (16, 10, 64, 64) and target.dtype == torch.uint8
    t = target.numpy() == 1
    er = t.copy()
    er[..., 1:, :] &= t[..., :-1, :]; er[..., :-1, :] &= t[..., 1:, :]
    er[..., :, 1:] &= t[..., :, :-1]; er[..., :, :-1] &= t[..., :, 1:]
    er[..., 0, :] = er[..., -1, :] = False; er[..., :, 0] = er[..., :, -1] = False
    ts, _, tg = hip.lv_measure(target.cuda())
    ridx, rval = hip.lv_ef(tg[..., 1], ts[..., 0])
    pidx, pval = hip.lv_ef(tg[..., 1], ts[..., 0], pick_vol=tg[..., 1], pick_npix=ts[..., 0])
    assert torch.equal(ridx, pidx) and torch.equal(rval, pval)
    assert (ridx[:, 2] == 10).all() and (rval[:, 2] > 0.2).all() and (rval[:, 2] < 0.9).all()       # areas pulsate by +-18 %
    sums = hip.ef_summary(pval[:, 2], rval[:, 2], ridx[:, 0] >= 0)
    st = hip.ef_stats(sums)
    assert st["clips_with_ef"] == 16 and st["ef_mae"] == 0.0 and st["ef_bias"] == 0.0
    es, _, eg = hip.lv_measure(torch.from_numpy(er.astype(np.uint8)).cuda())
    eidx, evals = hip.lv_ef(eg[..., 1], es[..., 0], pick_vol=tg[..., 1], pick_npix=ts[..., 0])
    assert torch.equal(eidx[:, :2], ridx[:, :2])
    assert (evals[:, 0] < rval[:, 0]).all() and (evals[:, 0] > 0).all()
