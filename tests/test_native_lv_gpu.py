"""gdkvm_lv_measure_native on the device against tests/native_lv_reference.py, on poisoned and guarded outputs (tests/poisoned_buffers.py):
the integers of steps 1 and 2 equal, the axis within one unit (a moved rint tie), and with the axis the device reported everything behind it
-- stats, disks, every word of the band rows -- exact and geom bit-equal.  The shapes sit on both sides of every published launch constant
and at the ends of the integer widths the header states (sides of 2048); uniform clips are compared bit for bit with gdkvm_lv_measure_mm
on the same bytes, doubles included, and ops.lv_ef and ops.lv_biplane take the records unchanged."""
import functools

import numpy as np
import pytest
import torch

from tests import native_lv_reference as R
from tests.poisoned_buffers import poisoned
from tests.test_native_lv_cpu import extreme_frames

pytestmark = pytest.mark.gpu
BAND = R.BAND_ROWS


def _run(ops, clips, spacing, D=20, cls=1, pad=1, byte=0x5A):
    """(stats, disks, geom, bands) as numpy from the device for lists of [T, h0, w0]; the mask starts `pad` bytes into a larger buffer whose
    other bytes are of the class.  Every output sits in a poisoned, guarded buffer: no word is left unwritten, no guard byte is touched."""
    flat, sizes = R.pack(clips)
    buf = torch.full((flat.size + pad + 5,), cls, dtype=torch.uint8, device="cuda")
    buf[pad:pad + flat.size] = torch.from_numpy(flat).cuda()
    with poisoned(byte) as ps:
        got = ops.lv_measure_native(buf[pad:pad + flat.size], sizes, int(clips[0].shape[0]), [tuple(s) for s in spacing], cls=cls, disks=D,
                                    want_bands=True)
        ps.check_guards()
        assert len(ps.outputs()) == 4
        for t in got:
            assert not bool(ps.unwritten(t).any()), "an output word still holds the poison"
    nb = int(clips[0].shape[0]) * sum((h + BAND - 1) // BAND for h, _ in sizes)
    assert [tuple(t.shape) for t in got] == [(len(clips), clips[0].shape[0], 12), (len(clips), clips[0].shape[0], D),
                                             (len(clips), clips[0].shape[0], 6), (nb, 8 + D)]
    return tuple(t.cpu().numpy() for t in got)


def _check(clips, spacing, got, D=20, cls=1):
    """The header's convention against the reference; no frame is left out."""
    stats, disks, geom, bands = got
    T = clips[0].shape[0]
    axes = [[None] * T for _ in clips]
    for b in range(len(clips)):
        for t in range(T):
            s = [int(v) for v in stats[b, t]]
            if s[0] == 0:
                continue                                      # (the reference then takes its own axis: a frame with pixels cannot match zeros)
            Vx, Vy, E, k = R.axis(*s[:6], int(spacing[b][0]), int(spacing[b][1]))
            assert abs(s[6] - Vx) <= 1 and abs(s[7] - Vy) <= 1 and abs(s[11] - E) <= 1, (b, t, s, (Vx, Vy, E))
            assert abs(float(geom[b, t, 4]) - k) <= 1e-12 * k, (b, t, geom[b, t, 4], k)
            axes[b][t] = (s[6], s[7], s[11], float(geom[b, t, 4]))
    want = R.records(clips, spacing, cls, D, axes)
    for name, g, w in zip(("stats", "disks", "geom", "bands"), got, want):
        assert g.shape == w.shape and np.array_equal(g.view(np.int64), w.view(np.int64)), (name, np.argwhere(g.view(np.int64) != w.view(np.int64))[:5])
    return want


def _ellipse(h, w, cy, cx, a, b, deg):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    th = np.radians(deg)
    al, ac = (xx - cx * w) * np.sin(th) + (yy - cy * h) * np.cos(th), (xx - cx * w) * np.cos(th) - (yy - cy * h) * np.sin(th)
    return ((al / (a * h)) ** 2 + (ac / (b * w)) ** 2 <= 1.0).astype(np.uint8)


def test_the_smallest_frames_and_the_degenerate_sets(hip):
    """1 x 1, 1 x 7 and 7 x 1 frames; per clip a class that fills the frame, a one-pixel class and an empty frame; other bytes are no class"""
    sizes = [(1, 1), (1, 7), (7, 1), (5, 9)]
    clips = []
    for h, w in sizes:
        c = np.zeros((3, h, w), np.uint8)
        c[0] = 1
        c[1, h // 2, w - 1] = 1
        c[2] = 255
        clips.append(c)
    sp = [(1, 4095), (4095, 1), (4095, 4095), (300, 450)]
    got = _run(hip, clips, sp)
    _check(clips, sp, got)
    assert not got[0][:, 2].any() and not got[1][:, 2].any() and not got[2][:, 2].any()        # the empty frames: all 0
    assert [int(v) for v in got[0][1, 0, :3]] == [7, 21, 0]


@pytest.mark.parametrize("h0,w0", [(BAND - 1, 37), (BAND, 21), (BAND + 1, 45), (2 * BAND + 1, 29)])
def test_both_sides_of_the_band(hip, h0, w0):
    """One band, one full band, two and three; w0 odd, so frames start at odd addresses.  Frame 1 has the class in the last band only,
    frame 2 in the first and the last band (h0 = 2 BAND + 1: an empty band between two occupied ones)."""
    rng = np.random.default_rng(h0 * 100 + w0)
    c = np.zeros((3, h0, w0), np.uint8)
    c[0] = rng.random((h0, w0)) < 0.4
    last = (h0 - 1) // BAND * BAND
    c[1, last:, 3:w0 - 2] = 1
    c[2, 2:6, 1:9] = 1
    c[2, last:, 5:11] = 1
    for sp in ((300, 450), (1000, 1000)):
        got = _run(hip, [c], [sp])
        _check([c], [sp], got)
    bands = got[3].reshape(3, -1, 28)
    if h0 > BAND:
        assert (bands[1, :-1, :6] == 0).all() and (bands[1, :-1, 6] == R.I64_MAX).all() and (bands[1, :-1, 7] == R.I64_MIN).all()
        assert not bands[1, :-1, 8:].any() and bands[1, -1, 0] > 0
    if h0 == 2 * BAND + 1:
        assert bands[2, 0, 0] == 32 and bands[2, 1, 0] == 0 and bands[2, 2, 0] == 6 and bands[2, 1, 6] == R.I64_MAX


@functools.lru_cache(maxsize=None)
def _ragged():
    sizes = [(47, 61), (70, 45), (33, 90)]
    clips = []
    for b, (h, w) in enumerate(sizes):
        c = np.zeros((3, h, w), np.uint8)
        for t in range(3):
            c[t] = _ellipse(h, w, 0.5 + 0.02 * b, 0.47, 0.36 - 0.04 * t, 0.2 - 0.02 * t, 25 * b + 10 * t)
            c[t][c[t] == 0] = 2 * (((np.arange(h)[:, None] + np.arange(w)[None, :]) % 5) == 0)[c[t] == 0]
        clips.append(c)
    return clips, [(300, 450), (1, 4095), (4095, 1)]


@pytest.mark.parametrize("D", [1, 20, 64])
def test_ragged_batch_and_every_clip_alone(hip, D):
    clips, sp = _ragged()
    got = _run(hip, clips, sp, D=D)
    want = _check(clips, sp, got, D=D)
    assert (want[0][..., 0] > 50).all()
    rows = 0
    for b, c in enumerate(clips):                             # no record depends on what else is in the batch
        alone = _run(hip, [c], sp[b:b + 1], D=D, pad=b)
        n = 3 * ((c.shape[1] + BAND - 1) // BAND)
        for k in range(3):
            assert np.array_equal(alone[k][0].view(np.int64), got[k][b].view(np.int64)), (b, k)
        assert np.array_equal(alone[3], got[3][rows:rows + n])
        rows += n
    if D == 20:
        other = _run(hip, clips, sp, D=D, cls=2)
        _check(clips, sp, other, D=D, cls=2)


def test_more_clips_than_a_launch(hip):
    clips_n = hip.LV_NATIVE_CLIPS + 1
    rng = np.random.default_rng(5)
    clips = [(rng.random((2, 3, 5)) < 0.6).astype(np.uint8) for _ in range(clips_n)]
    sp = [(1 + 37 * b, 4095 - 11 * b) for b in range(clips_n)]
    _check(clips, sp, _run(hip, clips, sp))


def test_more_items_than_the_workgroup_cap(hip):
    """64 clips x 65 frames of 2 x 2: more (frame, band) items than GDKVM_LV_NATIVE_MAX_WG in every kernel of the launch"""
    frames = 65
    assert hip.LV_NATIVE_CLIPS * frames > hip.LV_NATIVE_MAX_WG
    rng = np.random.default_rng(6)
    clips = [(rng.random((frames, 2, 2)) < 0.6).astype(np.uint8) for _ in range(hip.LV_NATIVE_CLIPS)]
    sp = [(300 + b, 450 - b) for b in range(hip.LV_NATIVE_CLIPS)]
    _check(clips, sp, _run(hip, clips, sp, D=3), D=3)


@pytest.mark.parametrize("which", range(5), ids=["full", "sides", "diagonal", "2x2048", "2048x2"])
def test_the_width_of_the_words(hip, which):
    """The width traps, one frame each: the largest A and a 32-bit n x (the full 2048 x 2048 frame), the outer 512 columns on each side,
    the largest L (a one-pixel diagonal at 4095 x 1 um), and the two thinnest frames of the longest side."""
    name, m, sp = extreme_frames()[which]
    got = _run(hip, [m[None]], [sp])
    want = _check([m[None]], [sp], got)
    assert int(want[0][0, 0, 0]) == int((m == 1).sum()) > 0
    if name == "full":
        assert int(got[0][0, 0, 0]) * 2047 > 1 << 32 and got[3].shape == (2048 // BAND, 28)


@pytest.mark.parametrize("h,w,clips,T", [(112, 112, 2, 3), (37, 53, 2, 3), (1024, 1024, 1, 1)])
def test_bit_equal_with_lv_measure_mm_on_uniform_clips(hip, h, w, clips, T):
    """Uniform clips packed ragged against gdkvm_lv_measure_mm on the same bytes (its register form, and at 1024 x 1024 the form that reads
    its vectors again): stats, disks and geom bit for bit, and ops.lv_ef on both gives the same bytes."""
    ops = hip
    frames = np.stack([np.stack([_ellipse(h, w, 0.5, 0.48 + 0.01 * b, 0.38 - 0.03 * t, 0.21 - 0.02 * t, 20 + 30 * b + 7 * t) for t in range(T)])
                       for b in range(clips)])
    frames[:, :, 0, 0] = 2
    sp = [(308, 154), (471, 333)][:clips]
    dev = torch.from_numpy(frames).cuda()
    spt = torch.tensor(sp, dtype=torch.int32, device="cuda")[:, None, :]
    for cls, D in ((1, 20), (2, 7)):
        old = ops.lv_measure_mm(dev, spt, cls=cls, disks=D)
        with poisoned(0xFF) as ps:
            new = ops.lv_measure_native(dev.reshape(-1), [(h, w)] * clips, T, sp, cls=cls, disks=D)
            ps.check_guards()
        for a, b in zip(old, new):
            assert a.shape == b.shape and torch.equal(a.view(torch.int64), b.view(torch.int64))
        assert int(old[0][..., 0].min()) > 0
        if T > 1:
            e_old = ops.lv_ef(old[2][..., 1], old[0][..., 0])
            e_new = ops.lv_ef(new[2][..., 1], new[0][..., 0])
            assert torch.equal(e_old[0], e_new[0]) and torch.equal(e_old[1].view(torch.int64), e_new[1].view(torch.int64))
            assert int(e_old[0][:, 0].min()) >= 0
    if h == 37:                                               # the small one also against the reference
        clips_np = [frames[b] for b in range(clips)]
        _check(clips_np, sp, _run(ops, clips_np, sp))


def test_two_calls_give_equal_bytes(hip):
    clips, sp = _ragged()
    a = _run(hip, clips, sp, byte=0x5A)
    b = _run(hip, clips, sp, byte=0xFF, pad=2)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int64), y.view(np.int64))


def test_lv_biplane_takes_the_native_records(hip):
    """A uniform 2CH / 4CH pair per patient measured through the native entry, with native_spacing_frames: bit for bit the grid path"""
    ops = hip
    h, w, T = 96, 80, 4
    views = np.stack([np.stack([_ellipse(h, w, 0.5, 0.5, 0.4 - 0.03 * t, 0.2 + 0.02 * v - 0.02 * t, 5 + 9 * v) for t in range(T)]) for v in range(4)])
    sp = [(308, 154), (300, 300), (154, 308), (471, 333)]
    pairs = torch.tensor([[0, 1], [2, 3], [1, 0]], dtype=torch.int32)
    dev = torch.from_numpy(views).cuda()
    spt = torch.tensor(sp, dtype=torch.int32, device="cuda")[:, None, :]
    grid = ops.lv_biplane(*ops.lv_measure_mm(dev, spt), spt, pairs)
    frames_sp = ops.native_spacing_frames(sp, T, dev.device)
    assert frames_sp.dtype == torch.int32 and tuple(frames_sp.shape) == (4, T, 2) and torch.equal(frames_sp, spt.expand(4, T, 2))
    native = ops.lv_biplane(*ops.lv_measure_native(dev.reshape(-1), [(h, w)] * 4, T, sp), frames_sp, pairs)
    assert torch.equal(grid[0].view(torch.int64), native[0].view(torch.int64)) and torch.equal(grid[1], native[1])
    assert float(grid[0][..., 0].min()) > 0


def test_refusals_on_the_device(hip):
    ops = hip
    m = torch.zeros(2 * (30 + 21), dtype=torch.uint8, device="cuda")
    sizes, sp = [(5, 6), (7, 3)], [(300, 200), (100, 100)]
    with poisoned(0x5A) as ps:
        with pytest.raises(ops.GdkvmError, match="outside 1..2048"):
            ops.lv_measure_native(m, [(5, 6), (7, 2049)], 2, sp)
        with pytest.raises(ops.GdkvmError, match="outside 1..4095"):
            ops.lv_measure_native(m, sizes, 2, [(300, 200), (100, 4096)])
        with pytest.raises(ops.GdkvmError, match="at least 102 bytes"):
            ops.lv_measure_native(m[:-1], sizes, 2, sp)
        assert not ps.records and not ps.calls                # refused before anything was allocated or launched
    stats, disks, geom = ops.lv_measure_native(m[:0], [], 2, [])
    assert tuple(stats.shape) == (0, 2, 12) and tuple(disks.shape) == (0, 2, 20) and tuple(geom.shape) == (0, 2, 6)
