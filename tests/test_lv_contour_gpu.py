"""gdkvm_lv_contour on the device against tests/contour_reference.py: every word of the record bit for bit, on outputs that sit poisoned between
guard bytes (tests/poisoned_buffers.py), so a word that was never written or a store past `rec` shows.  The shapes straddle what the kernel
branches on: the bit-plane word (pixel x is bit x + 1 of its row, so rows of 62 and 63 pixels end one word and start the next), the band of rows,
frames that start at odd byte addresses, and the frame's border, where a position outside reads as byte 0."""
import ctypes
import re
import os

import numpy as np
import pytest
import torch

from tests import contour_reference as R
from tests import poisoned_buffers as pb

pytestmark = pytest.mark.gpu

BAND, WORD = R.BAND_ROWS, R.WORD_BITS
_HDR = open(os.path.join(pb.ROOT, "include", "gdkvm.h")).read()
ERR_SHAPE = int(re.search(r"GDKVM_ERR_SHAPE = (-?\d+)", _HDR).group(1))
ERR_ARG = int(re.search(r"GDKVM_ERR_ARG = (-?\d+)", _HDR).group(1))
BYTES = np.array([0, 1, 2, 3, 4, 40, 255], np.uint8)


def test_the_constants_are_the_headers():
    from gdkvm_amd import ops
    assert int(re.search(r"#define GDKVM_LV_CONTOUR_BAND_ROWS (\d+)", _HDR).group(1)) == BAND == ops.LV_CONTOUR_BAND_ROWS
    assert int(re.search(r"#define GDKVM_LV_CONTOUR_WORD_BITS (\d+)", _HDR).group(1)) == WORD == ops.LV_CONTOUR_WORD_BITS


def _labels(F, H, W, seed, edges=True):
    """Random label frames of blocks (so that every class has long borders with every other) and speckle over the bytes {0..4, 40, 255},
    the class 1 on all four edges of the frame."""
    rng = np.random.default_rng(seed)
    bh, bw = max(H // 5, 1), max(W // 5, 1)
    coarse = rng.choice(BYTES, size=(F, -(-H // bh), -(-W // bw)), p=[0.2, 0.3, 0.15, 0.15, 0.1, 0.05, 0.05])
    m = np.repeat(np.repeat(coarse, bh, axis=1), bw, axis=2)[:, :H, :W].copy()
    sp = rng.random((F, H, W))
    m[sp < 0.08] = rng.choice(BYTES, size=int((sp < 0.08).sum()))
    if edges:
        m[:, 0, ::2] = 1; m[:, H - 1, 1::2] = 1; m[:, ::2, 0] = 1; m[:, 1::2, W - 1] = 1
        m[:, 0, 0] = 1; m[:, H - 1, W - 1] = 1
    return m


def _device_view(frames, off):
    """The frames on the device in a buffer of class bytes, starting `off` bytes behind a 16-byte boundary: no byte around them may count"""
    n = frames.size
    buf = torch.full((n + 48,), 1, dtype=torch.uint8, device="cuda")
    view = buf[off:off + n].view(*frames.shape)
    view.copy_(torch.from_numpy(frames))
    assert view.data_ptr() % 16 == off % 16
    return view


def _check(ops, frames, cls=1, wall=(2,), base=(3,), spacing=None, off=0, byte=0x5A):
    """Run under poison and guards and compare with the reference; spacing: None, (ry, rx) or an int array [F, 2].  Returns the record."""
    view = _device_view(frames, off)
    sp = None if spacing is None else torch.tensor(np.broadcast_to(np.asarray(spacing, np.int32), (frames.shape[0], 2)).copy(), dtype=torch.int32)
    with pb.poisoned(byte) as p:
        rec = ops.lv_contour(view, cls=cls, wall=wall, base=base, spacing_um=sp)
        torch.cuda.synchronize()
        assert rec.shape == frames.shape[:-2] + (16,) and rec.dtype == torch.int64
        assert not bool(p.unwritten(rec).any()), "a word of rec was never written"
        p.check_guards()
    want = R.contour_ref_frames(frames.reshape((-1,) + frames.shape[-2:]), cls, wall, base, spacing)
    got = rec.cpu().numpy().reshape(-1, 16)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (frames.shape, cls, wall, base, spacing, off, bad[:8].tolist(), got[bad[0][0]].tolist(), want[bad[0][0]].tolist())
    return got


@pytest.mark.parametrize("H,W,offs", [(7, 9, (1, 5)), (13, 17, (3, 15))])
def test_three_small_frames_at_odd_byte_offsets(hip, H, W, offs):
    assert (H * W) % 16 != 0
    frames = _labels(3, H, W, seed=H)
    for off in offs:
        got = _check(hip, frames, off=off)
        assert (got[:, 0] > 0).all() and (got[:, 5:9].sum(1) > 0).all()
    _check(hip, frames, spacing=(468, 330), off=offs[0])


@pytest.mark.parametrize("H,W", [(1, 1), (1, 37), (29, 1), (1, 130), (130, 1), (2, 2)])
def test_one_row_and_one_column(hip, H, W):
    frames = _labels(2, H, W, seed=H + W)
    _check(hip, frames, off=1)
    _check(hip, frames, wall=(0, 2), base=(3, 4))
    full = np.full((1, H, W), 1, np.uint8)                       # the class alone: every interface is with the outside
    got = _check(hip, full, wall=(2,), base=(0,))
    assert got[0, 5] == 2 * H and got[0, 6] == 2 * W


@pytest.mark.parametrize("W", [WORD - 3, WORD - 2, WORD - 1, WORD, WORD + 1, 2 * WORD - 2, 2 * WORD - 1, 2 * WORD, 2 * WORD + 1])
def test_widths_around_the_plane_word(hip, W):
    frames = _labels(2, 5, W, seed=W)
    frames[1, :, W - 2:] = 1                                     # the class in the row's last pixels, next to the halo column
    frames[1, 2, :] = 3
    _check(hip, frames, off=7)
    _check(hip, frames, wall=(0,), base=(3,), off=2)


@pytest.mark.parametrize("H", [BAND - 1, BAND, BAND + 1, 2 * BAND, 2 * BAND + 1])
def test_heights_around_the_band(hip, H):
    W = 21
    frames = _labels(3, H, W, seed=H)
    # an interface that lies between the first band's last row and the row behind it, and one inside the band's last row
    frames[1] = 0
    frames[1, :BAND, 3:15] = 1
    frames[1, BAND:, 3:15] = 2
    last = min(BAND, H) - 1
    frames[1, last, 8:11] = 3
    frames[1, BAND:, 15:] = 3
    frames[2] = 2
    frames[2, last:, :] = 3
    frames[2, min(BAND, H - 1):, 5:9] = 1                        # the class starts in the second band's first row (if there is one)
    _check(hip, frames, off=9)
    _check(hip, frames, spacing=(330, 468))


def test_one_frame_of_1024_by_1024(hip):
    frames = _labels(1, 1024, 1024, seed=1)
    yy, xx = np.mgrid[0:1024, 0:1024]
    frames[0][(yy - 500) ** 2 + (xx - 520) ** 2 < 300 ** 2] = 1  # a large body of the class beside the blocks
    got = _check(hip, frames, spacing=(4095, 1))
    assert got[0, 0] > 250000 and got[0, 14] > 0


@pytest.mark.parametrize("wall,base", [((0, 2), (3,)), ((2,), (0, 3)), ((2,), (3,))])
def test_the_class_on_all_four_edges(hip, wall, base):
    frames = _labels(2, 19, 23, seed=4)
    frames[1] = 1                                                # nothing but the class: only the outside can be a neighbour
    got = _check(hip, frames, wall=wall, base=base, off=3)
    ring = [2 * 19, 2 * 23, 2 * (19 + 23) - 2, 2 * (19 + 23) - 2]
    assert got[1, 1:5].tolist() == (ring if 0 in wall else [0] * 4) and got[1, 5:9].tolist() == (ring if 0 in base else [0] * 4)


def test_bytes_in_no_set(hip):
    frames = np.full((3, 11, 14), 255, np.uint8)
    frames[0, 3:8, 4:10] = 1                                     # neighbours 255 only
    frames[1] = 40; frames[1, 3:8, 4:10] = 1; frames[1, 2, 4:10] = 2      # 40 = 32 + 8: no member of a set that holds 8
    frames[2] = 33; frames[2, 5, 5] = 1; frames[2, 5, 6] = 34
    got = _check(hip, frames, wall=(2, 8), base=(3,), off=5)
    assert got[0, 1:9].tolist() == [0] * 8 and got[1, 1:5].tolist() == [0, 6, 5, 5] and not got[2, 1:9].any()
    _check(hip, frames, cls=31, wall=(1,), base=(2,))            # an absent class of the largest number


def test_an_empty_class_and_no_base_interface(hip):
    frames = _labels(3, 17, 16, seed=9, edges=False)
    frames[0][frames[0] == 1] = 0                                # no pixel of the class
    frames[1][frames[1] == 3] = 4                                # the class, and no base byte in the frame
    got = _check(hip, frames, off=11)
    assert got[0].tolist() == [0] * 11 + [-1, -1, -1, 0, 0]
    assert got[1, 0] > 0 and got[1, 1:5].sum() > 0 and got[1, 5:].tolist() == [0] * 6 + [-1, -1, -1, 0, 0]
    assert got[2, 5] + got[2, 6] > 0 and got[2, 13] >= 0


def test_an_apex_tie_goes_to_the_smallest_index(hip):
    H, W = 15, 21
    m = np.zeros((1, H, W), np.uint8)
    m[0, 3:12, 4:17] = 1                                         # a rectangle, the base in the middle of its upper edge: the two lower
    m[0, 2, 9:12] = 3                                            # corners are equally far
    m[0][(m[0] == 0)] = 2
    got = _check(hip, m)
    assert got[0, 11] == 2 * 10 and got[0, 13] == 11 * W + 4     # bx2 on the axis of symmetry; the LEFT lower corner
    d2 = lambda y, x: (2 * y - int(got[0, 12])) ** 2 + (2 * x - int(got[0, 11])) ** 2
    assert d2(11, 4) == d2(11, 16) == got[0, 14]


def test_a_spacing_moves_the_apex(hip):
    H, W = 24, 40
    m = np.full((1, H, W), 2, np.uint8)
    m[0, 4:6, 5:30] = 1                                          # an arm of 24 pixels along the row of the base ...
    m[0, 4:16, 5:7] = 1                                          # ... and one of 11 pixels down from it
    m[0, 3, 5:7] = 3
    px = R.contour_ref(m[0])
    mm = R.contour_ref(m[0], spacing=(4000, 1000))
    assert px[13] // W == 5 and px[13] % W == 29 and mm[13] // W == 15      # the case does what it is for
    _check(hip, m)
    got = _check(hip, m, spacing=(4000, 1000), off=13)
    assert got[0, 13] == mm[13] != px[13]
    _check(hip, m, spacing=(1, 1))                               # a spacing of one is the NULL spacing
    assert R.contour_ref(m[0], spacing=(1, 1)) == px


def test_a_device_spacing_out_of_range_gives_minus_one_records(hip):
    frames = _labels(4, 12, 13, seed=2)
    sp = np.array([[330, 468], [0, 468], [330, 4096], [4095, 1]], np.int32)
    view = _device_view(frames, 1)
    for byte in (0x5A, 0x00):                                    # (-1 is the 0xFF pattern itself)
        with pb.poisoned(byte) as p:
            rec = hip.lv_contour(view, spacing_um=torch.from_numpy(sp).cuda())
            torch.cuda.synchronize()
            assert not bool(p.unwritten(rec).any()) or byte == 0x00
            p.check_guards()
        got = rec.cpu().numpy()
        assert (got[1] == -1).all() and (got[2] == -1).all()
        assert got.tolist() == R.contour_ref_frames(frames, spacing=sp).tolist()
    lengths = hip.contour_lengths(rec, torch.from_numpy(sp).cuda()).cpu().numpy()
    assert (lengths[1:3] == -1.0).all()
    for f in (0, 3):
        assert np.allclose(lengths[f], R.lengths_ref(got[f], sp[f]), rtol=1e-12, atol=0.0)
    with pytest.raises(hip.GdkvmError, match="spacing_um outside"):                      # a host tensor is refused instead
        hip.lv_contour(view, spacing_um=torch.from_numpy(sp))


def test_two_calls_are_bit_equal_and_leading_dimensions_are_kept(hip):
    frames = _labels(6, 70, 67, seed=6)
    dev = torch.from_numpy(frames).cuda()
    a, b = hip.lv_contour(dev), hip.lv_contour(dev)
    c = hip.lv_contour(dev.view(2, 3, 70, 67))
    assert torch.equal(a, b) and c.shape == (2, 3, 16) and torch.equal(c.view(6, 16), a)
    assert hip.lv_contour(dev[:0]).shape == (0, 16)
    cpu = hip.lv_contour(torch.from_numpy(frames))               # the host rule of the same wrapper
    assert torch.equal(cpu, a.cpu())


def test_bad_arguments_return_their_code_and_leave_rec_alone(hip):
    lib = hip.load()
    mask = torch.ones(2 * 8 * 8 + 16, dtype=torch.uint8, device="cuda")
    rec = torch.full((2 * 16 + 2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    sp = torch.full((4,), 300, dtype=torch.int32, device="cuda")
    good = dict(mask=mask.data_ptr(), sp=None, rec=rec.data_ptr(), frames=2, H=8, W=8, cls=1, wall=4, base=8)

    def call(**kw):
        a = dict(good, **kw)
        return lib.gdkvm_lv_contour(a["mask"], a["sp"], a["rec"], a["frames"], a["H"], a["W"], a["cls"], a["wall"], a["base"], None)

    for kw in (dict(H=0), dict(W=1025), dict(H=1025), dict(frames=-1)):
        assert call(**kw) == ERR_SHAPE and b"lv_contour" in lib.gdkvm_last_error(), kw
    for kw in (dict(cls=-1), dict(cls=32), dict(cls=255), dict(wall=0), dict(wall=4, base=4 | 8), dict(wall=2 | 4), dict(base=2),
               dict(mask=None), dict(rec=None), dict(rec=rec.data_ptr() + 8), dict(sp=sp.data_ptr() + 2)):
        assert call(**kw) == ERR_ARG and b"lv_contour" in lib.gdkvm_last_error(), kw
    assert call(frames=0, mask=None, rec=None) == 0              # nothing to do: no launch, no pointer is looked at
    torch.cuda.synchronize()
    assert bool((rec == 0x5A5A5A5A5A5A5A5A).all())
    assert call() == 0 and call(sp=sp.data_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((rec[:32] != 0x5A5A5A5A5A5A5A5A).all()) and bool((rec[32:] == 0x5A5A5A5A5A5A5A5A).all())
    assert ctypes.sizeof(ctypes.c_uint) == 4
