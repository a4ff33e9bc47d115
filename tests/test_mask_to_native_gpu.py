"""gdkvm_mask_to_native on the device against tests/native_reference.py, bit for bit: out and counts.  The shapes sit where the kernel can go
wrong rather than at the workload's size: the top-left half-pixel (floor division below zero), up- and down-scales that are no whole
ratio, single pixels on either side, native widths on both sides of a lane's run, odd h0 w0 (every later frame and clip then starts at
another alignment), clips of different sizes in one call, clip counts on both sides of the launcher's chunk, more work items than a launch
has workgroups, the 2^24 end of a vote's range, and every class count the launcher has a kernel for."""
import os
import re

import numpy as np
import pytest
import torch

from tests import native_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HDR = open(os.path.join(ROOT, "include", "gdkvm.h")).read()
_define = lambda name: int(re.search(r"#define GDKVM_MASK_TO_NATIVE_" + name + r" (\d+)", _HDR).group(1))
RUN, BAND_PIXELS, MAX_WG, CLIPS = _define("RUN"), _define("BAND_PIXELS"), _define("MAX_WG"), _define("CLIPS")
ERR_SHAPE = int(re.search(r"GDKVM_ERR_SHAPE = (-?\d+)", _HDR).group(1))


def _mask(rng, clips, T, H, W, ncls, p255=0.1):
    m = rng.integers(0, ncls, (clips, T, H, W)).astype(np.uint8)
    m[rng.random(m.shape) < p255] = 255
    return m


def _target(rng, total, ncls, p255=0.2):
    g = rng.integers(0, ncls, total).astype(np.uint8)
    g[rng.random(total) < p255] = 255
    return g


def _check(hip, m, sizes, ncls, seed=0, with_target=True):
    """out and counts of one call against the restatement; returns what the device gave"""
    rng = np.random.default_rng(seed)
    total = R.offsets(sizes, m.shape[1])[1]
    g = _target(rng, total, ncls) if with_target else None
    ref_out, ref_counts = R.mask_to_native(m, sizes, ncls, g)
    out, counts, offs = hip.mask_to_native(torch.from_numpy(m).cuda(), sizes, ncls, target=None if g is None else torch.from_numpy(g).cuda())
    assert offs == R.offsets(sizes, m.shape[1])[0]
    assert np.array_equal(out.cpu().numpy(), ref_out)
    if with_target:
        assert counts.dtype == torch.int32 and np.array_equal(counts.cpu().numpy(), ref_counts)
    else:
        assert counts is None
    return out, counts


# (H, W, h0, w0): identity, x2, x3, odd up-scale, down-scale, up-scale past one run, a single source pixel, a single native pixel
SIZES = [(8, 8, 8, 8), (8, 8, 16, 16), (8, 8, 24, 24), (7, 5, 11, 13), (16, 12, 5, 7), (16, 16, 23, 37), (1, 1, 4, 5), (4, 4, 1, 1),
         (112, 112, 300, 411)]


@pytest.mark.parametrize("shape", SIZES, ids=lambda s: "%dx%d_to_%dx%d" % s)
@pytest.mark.parametrize("ncls", [2, 4, 8])
def test_sizes_match_the_restatement(hip, shape, ncls):
    H, W, h0, w0 = shape
    m = _mask(np.random.default_rng(H * 31 + w0), 2, 3, H, W, ncls)
    out, _ = _check(hip, m, [(h0, w0), (h0, w0)], ncls)
    if (H, W) == (h0, w0):                                        # identity at equal sizes (bytes >= ncls are 255 here)
        assert np.array_equal(out.cpu().numpy(), m.reshape(-1))


@pytest.mark.parametrize("ncls", [3, 5, 6, 7])
def test_every_class_count_has_its_kernel(hip, ncls):
    _check(hip, _mask(np.random.default_rng(ncls), 2, 2, 9, 7, ncls), [(13, 17), (20, 9)], ncls)


@pytest.mark.parametrize("w0", [RUN - 1, RUN, RUN + 1, 63, 64, 65])
def test_widths_on_both_sides_of_a_run_with_odd_frames(hip, w0):
    h0 = 7 if w0 % 2 else 9
    sizes = [(h0, w0), (h0 + 2, w0)] if w0 % 2 else [(h0, w0 + 1), (h0, w0)]
    assert (sizes[0][0] * sizes[0][1]) % 2 == 1                   # every later frame and the second clip start misaligned
    _check(hip, _mask(np.random.default_rng(w0), 2, 3, 6, 6, 4), sizes, 4)


def test_clips_of_different_sizes_in_one_call(hip):
    rng = np.random.default_rng(5)
    for sizes in ([(129, 63), (3, 15), (40, 65), (5, 5)], [(5, 5), (3, 15), (40, 65), (129, 63)]):     # the largest first, and last
        _check(hip, _mask(rng, 4, 2, 9, 7, 4), sizes, 4)


def test_a_band_is_whole_rows_and_frames_have_several(hip):
    # 70 x 130 = 9100 pixels: bands of ceil(4096 / 130) = 32 rows, three of them, the last short; 700 x 3: one band of all rows
    assert -(-BAND_PIXELS // 130) == 32
    _check(hip, _mask(np.random.default_rng(6), 1, 2, 8, 8, 3), [(70, 130)], 3)
    _check(hip, _mask(np.random.default_rng(7), 1, 2, 3, 2, 3), [(700, 3)], 3)


@pytest.mark.parametrize("clips", [CLIPS - 1, CLIPS, CLIPS + 1, 2 * CLIPS + 1])
def test_the_chunk_walk_carries_the_offsets(hip, clips):
    sizes = [(1 + k % 5, 1 + k % 7) for k in range(clips)]
    _check(hip, _mask(np.random.default_rng(clips), clips, 2, 3, 4, 4), sizes, 4)


def test_more_items_than_workgroups(hip):
    # h0 <= 2048 and a band holds at least two rows of the widest frame, so ONE frame has at most 1024 bands and cannot reach the cap of
    # MAX_WG workgroups on its own (2048 x 2048 would take 4 MB per frame besides): the items are (clip, frame, band), and frames and clips
    # reach it.  One clip of MAX_WG + 4 tiny frames; and a full launch of clips whose first has two bands per frame (the second one row
    # short of nothing: a single row) while the others have one, so that the grid follows the first and every other clip's second item leaves.
    _check(hip, _mask(np.random.default_rng(8), 1, MAX_WG + 4, 1, 2, 2), [(2, 2)], 2)
    rows = -(-BAND_PIXELS // 33)
    sizes = [(rows + 1, 33)] + [(2 + k % 3, 3) for k in range(CLIPS - 1)]
    assert CLIPS * 33 * 2 > MAX_WG
    _check(hip, _mask(np.random.default_rng(9), CLIPS, 33, 5, 6, 2), sizes, 2)


def test_the_vote_range_end(hip):
    # 2 x 2 -> 2048 x 2048: the weights reach 4 h0 w0 = 2^24; and the narrowest tall frame
    _check(hip, _mask(np.random.default_rng(10), 1, 1, 2, 2, 2, p255=0.0), [(2048, 2048)], 2)
    _check(hip, _mask(np.random.default_rng(11), 1, 1, 3, 2, 4), [(2048, 3)], 4)


def test_unlabelled_bytes(hip):
    m = _mask(np.random.default_rng(12), 2, 2, 6, 5, 4, p255=0.5)
    m[1, 1] = 255                                                 # an all-255 source frame: nothing votes anywhere
    sizes = [(9, 11), (13, 7)]
    offs, total = R.offsets(sizes, 2)
    g = _target(np.random.default_rng(13), total, 4)
    g[offs[1]:offs[1] + 13 * 7] = 255                             # an all-255 target frame
    out, counts, _ = hip.mask_to_native(torch.from_numpy(m).cuda(), sizes, 4, target=torch.from_numpy(g).cuda())
    ref_out, ref_counts = R.mask_to_native(m, sizes, 4, g)
    assert np.array_equal(out.cpu().numpy(), ref_out) and np.array_equal(counts.cpu().numpy(), ref_counts)
    assert (counts[1, 0, :, 2] == 0).all() and (counts[1, 0, :, 0] == 0).all()
    assert (hip.native_frames(out, sizes, 2, 1)[1] == 255).all() and (counts[1, 1, :, :2] == 0).all()


def test_without_target_without_out_and_at_odd_offsets(hip):
    rng = np.random.default_rng(14)
    m = _mask(rng, 2, 2, 7, 5, 4)
    sizes = [(11, 13), (30, 17)]
    total = R.offsets(sizes, 2)[1]
    _check(hip, m, sizes, 4, with_target=False)
    g = _target(rng, total, 4)
    ref_out, ref_counts = R.mask_to_native(m, sizes, 4, g)
    md = torch.from_numpy(m).cuda()
    none, counts, _ = hip.mask_to_native(md, sizes, 4, target=torch.from_numpy(g).cuda(), want_out=False)
    assert none is None and np.array_equal(counts.cpu().numpy(), ref_counts)
    for o_shift, t_shift in ((3, 3), (0, 5), (7, 0)):
        obuf = torch.full((total + 32,), 0xAA, dtype=torch.uint8, device="cuda")
        tbuf = torch.zeros(total + 32, dtype=torch.uint8, device="cuda")
        tbuf[t_shift:t_shift + total] = torch.from_numpy(g).cuda()
        out, counts, _ = hip.mask_to_native(md, sizes, 4, target=tbuf[t_shift:t_shift + total], out=obuf[o_shift:o_shift + total])
        assert out.data_ptr() == obuf.data_ptr() + o_shift
        assert np.array_equal(out.cpu().numpy(), ref_out) and np.array_equal(counts.cpu().numpy(), ref_counts)
        assert (obuf[:o_shift] == 0xAA).all() and (obuf[o_shift + total:] == 0xAA).all()        # not a byte beside the masks
        none, counts, _ = hip.mask_to_native(md, sizes, 4, target=tbuf[t_shift:t_shift + total], want_out=False)
        assert np.array_equal(counts.cpu().numpy(), ref_counts)


def test_two_calls_give_identical_bytes(hip):
    rng = np.random.default_rng(15)
    m = torch.from_numpy(_mask(rng, 3, 4, 31, 29, 4)).cuda()
    sizes = [(97, 131), (60, 61), (200, 33)]
    g = torch.from_numpy(_target(rng, R.offsets(sizes, 4)[1], 4)).cuda()
    a, b = hip.mask_to_native(m, sizes, 4, target=g), hip.mask_to_native(m, sizes, 4, target=g)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_no_clips_is_no_launch(hip):
    out, counts, offs = hip.mask_to_native(torch.zeros((0, 2, 4, 4), dtype=torch.uint8, device="cuda"), [], 4)
    assert out.numel() == 0 and counts is None and offs == []


def test_bad_arguments_are_refused_before_any_launch(hip):
    lib = hip.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    clips, T, H, W, ncls = 2, 2, 4, 4, 4
    sizes = np.array([[5, 6], [7, 3]], np.int32)
    total = T * (30 + 21)
    mask = torch.zeros((clips, T, H, W), dtype=torch.uint8, device=dev)
    buf = torch.full((2 * total + 64,), 0x5A, dtype=torch.uint8, device=dev)
    out, target = buf[:total], buf[total + 16:2 * total + 16]
    cbuf = torch.full((clips * T * ncls * 3 + 8,), -7, dtype=torch.int32, device=dev)
    counts = cbuf[:clips * T * ncls * 3]
    assert counts.data_ptr() % 16 == 0 and mask.data_ptr() % 16 == 0

    def call(mask_p=mask.data_ptr(), sizes_a=sizes, target_p=target.data_ptr(), out_p=out.data_ptr(), counts_p=counts.data_ptr(),
             native_bytes=total, clips_=clips, T_=T, H_=H, W_=W, ncls_=ncls):
        return lib.gdkvm_mask_to_native(mask_p, None if sizes_a is None else sizes_a.ctypes.data, target_p, out_p, counts_p, native_bytes, None, 0,
                                        clips_, T_, H_, W_, ncls_, torch.cuda.current_stream(dev).cuda_stream)

    bad_size = lambda h0, w0: np.array([[5, 6], [h0, w0]], np.int32)
    cases = {"clips < 0": dict(clips_=-1), "T = 0": dict(T_=0), "H = 0": dict(H_=0), "W = 1025": dict(W_=1025), "ncls = 1": dict(ncls_=1),
             "ncls = 9": dict(ncls_=9), "h0 = 0": dict(sizes_a=bad_size(0, 3)), "w0 = 2049": dict(sizes_a=bad_size(7, 2049)),
             "h0 < 0": dict(sizes_a=bad_size(-4, 3)), "null mask": dict(mask_p=None), "null sizes": dict(sizes_a=None),
             "null counts": dict(counts_p=None), "misaligned counts": dict(counts_p=counts.data_ptr() + 4),
             "target without counts": dict(counts_p=None, out_p=None), "neither out nor target": dict(out_p=None, target_p=None),
             "short native_bytes": dict(native_bytes=total - 1), "out over mask": dict(out_p=mask.data_ptr()),
             "out over target": dict(out_p=target.data_ptr() + total - 1), "out into target": dict(out_p=target.data_ptr() - 1)}
    for name, kw in cases.items():
        assert call(**kw) == ERR_SHAPE, name
        assert b"mask_to_native" in lib.gdkvm_last_error(), name
    torch.cuda.synchronize()
    assert (buf == 0x5A).all() and (cbuf == -7).all() and (mask == 0).all()       # nothing was launched: not even the zeroing of counts
    assert call(clips_=0) == 0
    torch.cuda.synchronize()
    assert (buf == 0x5A).all() and (cbuf == -7).all()
    assert call() == 0                                            # and the same arguments, untouched, are fine
    torch.cuda.synchronize()
    assert (cbuf[:counts.numel()] != -7).all() and (cbuf[counts.numel():] == -7).all() and (out != 0x5A).any()


def test_wrapper_refuses_device_sizes(hip):
    m = torch.zeros((1, 1, 4, 4), dtype=torch.uint8, device="cuda")
    with pytest.raises(hip.GdkvmError, match="host integers"):
        hip.mask_to_native(m, torch.tensor([[4, 4]], device="cuda"), 2)
