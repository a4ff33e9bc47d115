"""gdkvm_surface_distance_native on the device against tests/native_surface_reference.py: exact equality of the int64 records on ragged
batches at every byte alignment, beyond the limits of gdkvm_surface_distance_mm (sides above 1024, the largest operand the isqrt ever sees),
on both sides of every published launch constant, on the degenerate sets, against the parent's kernel on uniform clips, and with a poisoned
workspace."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import native_surface_reference as NR
from tests.native_eval_fixture import _drawing

pytestmark = pytest.mark.gpu

SIZES = [(47, 61), (32, 32), (70, 45), (21, 90), (55, 54), (5, 7), (33, 31), (17, 65), (1, 1)]
SPACING = [(308, 154), (1, 4095), (4095, 1), (333, 471), (154, 308), (1000, 1000), (7, 3), (2048, 2047), (4095, 4095)]
T = 3


def _ops():
    from gdkvm_amd import ops
    ops.require_native()
    return ops


def _run(masks, targets, spacing, cls=1, pad=0):
    """records int64 [clips, T, 8] from the device for lists of [T, h0, w0]; pad: the buffers start `pad` bytes into a larger one"""
    ops = _ops()
    fm, sizes = NR.pack(masks)
    ft, _ = NR.pack(targets)
    gm = torch.full((fm.size + pad + 3,), cls, dtype=torch.uint8, device="cuda")        # (the bytes around the frames are of the class)
    gt = torch.full((ft.size + pad + 5,), cls, dtype=torch.uint8, device="cuda")
    gm[pad:pad + fm.size] = torch.from_numpy(fm).cuda()
    gt[pad:pad + ft.size] = torch.from_numpy(ft).cuda()
    out = ops.surface_distance_native(gm[pad:pad + fm.size], gt[pad:pad + ft.size], sizes, masks[0].shape[0], [tuple(s) for s in spacing], cls=cls)
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _ragged():
    masks, targets = [], []
    for b, (h0, w0) in enumerate(SIZES):
        m, g = np.zeros((T, h0, w0), np.uint8), np.zeros((T, h0, w0), np.uint8)
        for t in range(T):
            k = 1.0 - 0.08 * t
            g[t] = _drawing(h0, w0, 0.5 + 0.02 * b, 0.47, 0.27 * k, (0.17 + 0.01 * b) * k)
            m[t] = _drawing(h0, w0, 0.53 + 0.02 * b, 0.44, 0.25 * k, (0.19 + 0.01 * b) * k)
        masks.append(m)
        targets.append(g)
    masks[5][:, 1:4, 2:5] = 1                                 # the drawing leaves the smallest frames empty: a block and a pixel
    targets[5][:, 2, 5] = 1
    masks[8][:] = 1
    targets[8][:] = 1
    ref = NR.records(masks, targets, SPACING)
    ref.setflags(write=False)
    return masks, targets, ref


def test_ragged_batch_matches_the_reference_and_every_clip_alone(hip):
    masks, targets, ref = _ragged()
    assert (ref[:5, :, :2] > 0).all() and (ref[..., 2:4].max() > 0)          # the fixture does measure something
    got = _run(masks, targets, SPACING)
    assert np.array_equal(got, ref), (got - ref)
    for b in range(len(SIZES)):                               # no record depends on what else is in the batch
        alone = _run(masks[b:b + 1], targets[b:b + 1], SPACING[b:b + 1])
        assert np.array_equal(alone[0], ref[b]), b
    other = _run(masks, targets, SPACING, cls=2)
    assert np.array_equal(other, NR.records(masks, targets, SPACING, cls=2))


def _two_pixels(h0, w0):
    m, g = np.zeros((1, h0, w0), np.uint8), np.zeros((1, h0, w0), np.uint8)
    m[0, 0, 0] = 1
    g[0, h0 - 1, w0 - 1] = 1
    return m, g


def test_sides_beyond_1024_and_the_largest_operand(hip):
    for (h0, w0), (ry, rx) in (((1100, 3), (308, 154)), ((3, 1100), (154, 308))):
        m, g = _two_pixels(h0, w0)
        d2 = (ry * (h0 - 1)) ** 2 + (rx * (w0 - 1)) ** 2
        s = math.isqrt(d2 << 16)
        want = np.asarray([[[1, 1, d2, d2, s, s, d2, d2]]], np.int64)
        assert np.array_equal(NR.records([m], [g], [(ry, rx)]), want)
        assert np.array_equal(_run([m], [g], [(ry, rx)]), want), (h0, w0)
    d2 = (2047 * 4095) ** 2
    s = math.isqrt(d2 << 16)                                  # the largest operand of one axis
    for h0, w0 in ((2048, 1), (1, 2048)):
        m, g = _two_pixels(h0, w0)
        got = _run([m], [g], [(4095, 4095)])
        assert np.array_equal(got, np.asarray([[[1, 1, d2, d2, s, s, d2, d2]]], np.int64)), (h0, w0, got)
    # ... and of both: opposite corners of the largest frame the entry takes, d2 = 2 (2047 * 4095)^2, the bound include/gdkvm.h states
    m, g = _two_pixels(2048, 2048)
    d2 = 2 * (2047 * 4095) ** 2
    s = math.isqrt(d2 << 16)
    assert (d2 << 16) < 1 << 63
    assert np.array_equal(_run([m], [g], [(4095, 4095)]), np.asarray([[[1, 1, d2, d2, s, s, d2, d2]]], np.int64))


def _rect(h0, w0, y0, y1, x0, x1, frames=1):
    m = np.zeros((frames, h0, w0), np.uint8)
    m[:, y0:y1, x0:x1] = 1
    return m


@pytest.mark.parametrize("h0,w0", [(31, 63), (32, 64), (33, 65), (101, 70), (64, 129)])
def test_both_sides_of_the_band_and_of_the_strip(hip, h0, w0):
    """One band and two, one strip and two (three), a frame of four bands; the surfaces run along the band boundaries (rows 31 | 32, 63 | 64)
    and the strip boundary (columns 63 | 64) wherever the frame has them."""
    ops = _ops()
    B, S = ops.SURFACE_NATIVE_BAND_ROWS, ops.SURFACE_NATIVE_STRIP
    assert (B, S) == (32, 64)
    rng = np.random.default_rng(h0 * 100 + w0)
    masks = [_rect(h0, w0, B - 1 if h0 > B else 3, min(2 * B + 1, h0 - 1), 2, min(S + 1, w0)),          # edges on rows 31 and 64, column 64
             _rect(h0, w0, min(B, h0 - 2), h0, min(S - 1, w0 - 2), w0),                                  # first row 32, first column 63
             (rng.random((1, h0, w0)) < 0.3).astype(np.uint8)]
    targets = [_rect(h0, w0, 0, min(B, h0), 0, min(S, w0)),                                              # last row 31, last column 63
               _rect(h0, w0, 1, 2, 0, w0),
               (rng.random((1, h0, w0)) < 0.02).astype(np.uint8)]
    sp = [(300, 200), (150, 400), (1, 1)]
    assert np.array_equal(_run(masks, targets, sp), NR.records(masks, targets, sp))


def test_more_clips_than_a_launch_and_more_items_than_the_workgroup_cap(hip):
    ops = _ops()
    clips = ops.SURFACE_NATIVE_CLIPS + 1
    frames = 65                                               # 64 clips x 65 frames: the first launch has more items than MAX_WG in every kernel
    assert ops.SURFACE_NATIVE_CLIPS * frames > ops.SURFACE_NATIVE_MAX_WG
    rng = np.random.default_rng(5)
    sizes = [(1 + b % 3, 2 + b % 2) for b in range(clips)]
    masks = [(rng.random((frames, h, w)) < 0.5).astype(np.uint8) for h, w in sizes]
    targets = [(rng.random((frames, h, w)) < 0.5).astype(np.uint8) for h, w in sizes]
    sp = [(1 + 37 * b, 4095 - 11 * b) for b in range(clips)]
    got = _run(masks, targets, sp)
    assert np.array_equal(got, NR.records(masks, targets, sp))
    one = _run([m[:1] for m in masks], [g[:1] for g in targets], sp)              # T = 1
    assert np.array_equal(one, got[:, :1])


def test_degenerate_sets(hip):
    h0, w0 = 40, 40
    z = lambda: np.zeros((1, h0, w0), np.uint8)
    blob = _rect(h0, w0, 10, 30, 8, 25)
    full = np.ones((1, h0, w0), np.uint8)
    two = z(); two[0, 3, 4] = 1
    far = z(); far[0, 39, 0] = 1
    board = z(); board[0, (np.add.outer(np.arange(h0), np.arange(w0)) % 2) == 0] = 1
    other = np.full((1, h0, w0), 255, np.uint8); other[0, 20, 20] = 1
    pairs = [(z(), blob), (blob, z()), (z(), z()),            # the class absent from the mask, from the target, from both
             (full, blob), (blob, full), (full, full),        # the whole frame: its surface is the border ring
             (two, far),                                      # n = 2: lo = hi = 0
             (board, far), (far, board),                      # every pixel of the class is surface; long walks
             (other, blob)]                                   # other bytes are not the class
    masks, targets = [p[0] for p in pairs], [p[1] for p in pairs]
    sp = [(308, 154)] * len(pairs)
    ref = NR.records(masks, targets, sp)
    assert ref[3, 0, 0] == 2 * (h0 + w0) - 4 and ref[6, 0, 6] == ref[6, 0, 7] and ref[7, 0, 0] == h0 * w0 // 2
    assert np.array_equal(_run(masks, targets, sp), ref)
    # the last row of frame t and the first row of frame t + 1 full of the class: no adjacency across the frames of the ragged buffer
    m = np.zeros((3, 9, 11), np.uint8); m[0, 8, :] = 1; m[1, 0, :] = 1; m[1, 8, :] = 1; m[2, 0, :] = 1
    g = np.zeros((3, 9, 11), np.uint8); g[:, 4, 5] = 1
    ref = NR.records([m], [g], [(100, 100)])
    assert ref[0, 0, 0] == 11 and ref[0, 1, 0] == 22
    assert np.array_equal(_run([m], [g], [(100, 100)]), ref)


@pytest.mark.parametrize("h,w", [(24, 20), (150, 130)])
def test_bit_equal_with_surface_distance_mm_on_uniform_clips(hip, h, w):
    """Uniform clips packed ragged against the parent's kernel on the same bytes: its LDS form (24 x 20) and its workspace form (150 x 130 =
    19 500 pixels, above SURFACE_MM_LDS_PIXELS)."""
    from tests import surface_reference as S
    ops = _ops()
    assert (h * w > ops.SURFACE_MM_LDS_PIXELS) == (h == 150)
    clips, frames = 2, 3
    a = S.random_frames(clips * frames, h, w, seed=11).reshape(clips, frames, h, w)
    b = S.random_frames(clips * frames, h, w, seed=12).reshape(clips, frames, h, w)
    sp = [(308, 154), (471, 333)]
    ga, gb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    spt = torch.tensor(sp, dtype=torch.int32, device="cuda")[:, None, :].expand(clips, frames, 2).contiguous()
    for cls in (1, 2):
        old = ops.surface_distance_mm(ga, gb, spt, cls=cls)
        new = ops.surface_distance_native(ga.reshape(-1), gb.reshape(-1), [(h, w)] * clips, frames, sp, cls=cls)
        assert old.shape == new.shape and torch.equal(old, new)
        assert int(old[..., 0].min()) > 0


def test_poisoned_workspace_guards_and_repeatability(hip):
    ops = _ops()
    masks, targets, ref = _ragged()
    fm, sizes = NR.pack(masks)
    ft, _ = NR.pack(targets)
    clips, total, rows = len(sizes), fm.size, T * sum(h for h, _ in sizes)
    need = ops._bytes("gdkvm_surface_distance_native_workspace_bytes", torch.device("cuda", torch.cuda.current_device()), clips, T, total, rows)
    assert need > 0 and need % 16 == 0
    guard = 256
    ws = torch.full((need + guard,), 0xff, dtype=torch.uint8, device="cuda")
    surf = torch.full((clips * T * 8 + 32,), -7, dtype=torch.int64, device="cuda")
    gm, gt = torch.from_numpy(fm).cuda(), torch.from_numpy(ft).cuda()
    hs, hp = torch.tensor(sizes, dtype=torch.int32), torch.tensor(SPACING, dtype=torch.int32)
    got = []
    for _ in range(2):
        ops._call("gdkvm_surface_distance_native", gm.device, gm, gt, hs, hp, surf, total, ops._Ws(ws[:need]), clips, T, 1)
        got.append(surf[:clips * T * 8].cpu().numpy().reshape(clips, T, 8).copy())
        assert bool((ws[need:] == 0xff).all()) and bool((surf[clips * T * 8:] == -7).all())
        ws[:need] = 0x5a                                      # another poison for the second call
    assert np.array_equal(got[0], ref) and np.array_equal(got[1], ref)
    assert np.array_equal(_run(masks, targets, SPACING, pad=1), ref)          # mask and target one byte into a larger buffer
    with pytest.raises(ops.GdkvmError, match="workspace"):
        ops._call("gdkvm_surface_distance_native", gm.device, gm, gt, hs, hp, surf, total, ops._Ws(ws[:need - 16]), clips, T, 1)
