"""gdkvm_largest_component on the device against tests/cc_reference.py, bit for bit: the filtered mask and all eight info integers.  The shapes
sit where the kernel can go wrong rather than at the workload's size: both sides of the LDS / workspace split (15360 pixels), frames whose
H*W is no multiple of 16 (every frame after the first starts unaligned), one-pixel-wide frames, rows longer than a wave's vectors."""
import numpy as np
import pytest
import torch

from tests import cc_reference as C
from tests import lv_reference as R

pytestmark = pytest.mark.gpu

# (frames of the random recipe, H, W): the cfg2 mask; exactly the last LDS size and the first workspace size; the two sizes of the LV test
# above the split; H*W = 1740 and 195 (unaligned frames with heads and tails); one long row per 64 lanes; single rows / columns; one pixel
SHAPES = [(6, 112, 112), (2, 120, 128), (2, 121, 127), (2, 256, 256), (2, 320, 272), (4, 30, 58), (5, 15, 13), (2, 8, 1024), (3, 1, 37),
          (3, 37, 1), (1, 1, 1)]
ALL = [(conn, cls, fill) for conn in (4, 8) for cls in (1, 2) for fill in (0, 3)]
NCLS = 4


def _combos(H, W):
    """Every combination below 20000 pixels; above, two that still cover both connectivities, classes and fills (the Python reference takes
    a tenth of a second per large frame)."""
    return ALL if H * W < 20000 else [(4, 1, 0), (8, 2, 3)]


def _random_frames(F, H, W, seed):
    """The recipe of the LV test: unions of random rotated ellipses of classes 1 and 2, speckle of both, a patch of class 3 and one of 255."""
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


def _special_frames(H, W, cls, seed):
    """One frame per corner of the definition (degenerate but valid on the one-pixel-wide shapes)."""
    rng = np.random.default_rng(seed)
    z = lambda: np.zeros((H, W), np.uint8)
    box = lambda m, y0, y1, x0, x1: m.__setitem__((slice(min(y0, H - 1), min(y1, H)), slice(min(x0, W - 1), min(x1, W))), cls)
    fr = []
    for _ in range(2):                                           # just under the 4-connected percolation threshold: large, tortuous components
        m = z(); m[rng.random((H, W)) < 0.55] = cls; fr.append(m)
    fr.append(C.serpentine(H, W, cls))
    fr.append(C.spiral(H, W, cls))
    fr.append(C.checkerboard(H, W, cls))
    fr.append(np.full((H, W), cls, np.uint8))                    # the full frame, then the empty one: pixels of the class in frame f only
    fr.append(z())
    m = z(); box(m, 1, 3, 1, 3); box(m, 3, 6, 3, 6); fr.append(m)                            # touch only diagonally (down-right)
    m = z(); box(m, 1, 3, 4, 6); box(m, 3, 5, 2, 4); fr.append(m)                            # ... and down-left: the up-right neighbour
    m = z(); box(m, 1, 3, 8, 10); box(m, 2, 6, 2, 3); box(m, 8, 10, 5, 7); fr.append(m)      # a tie: the first blob along the rows wins
    m = z(); box(m, 2, 4, 8, 10); box(m, 1, 5, 2, 3); box(m, 8, 10, 5, 7); fr.append(m)      # a tie: the winner is the blob a row-major scan COMPLETES last
    m = z(); box(m, 1, 3, 8, 10); box(m, 1, 5, 2, 3); box(m, 8, 11, 5, 7); fr.append(m)      # a later, larger blob beats both
    m = z(); m[:, W - 1] = cls; m[:, 0] = cls; m[H // 2, :] = 255 - cls; fr.append(m)        # (W - 1, y) beside (0, y + 1) in memory, every row
    m = z(); m[H - 1, W - 1] = cls; m[0, 0] = cls; box(m, 0, 2, 3, 6); fr.append(m)          # the last byte of this frame ...
    m = z(); m[0, 0] = cls; m[H - 1, W - 1] = cls; box(m, H - 3, H - 1, 0, 2); fr.append(m)  # ... and the first byte of the next
    m = np.full((H, W), 255, np.uint8); box(m, 1, 4, 1, 3); m[H - 1, W - 1] = cls; fr.append(m)
    return np.stack(fr)


_CACHE = {}


def _case(F, H, W, conn, cls, fill):
    """(frames, target, reference out, reference info) -- computed once per case and shared, never modified."""
    key = (F, H, W, conn, cls, fill)
    if key not in _CACHE:
        frames = np.concatenate([_random_frames(F, H, W, seed=H * 1000 + W), _special_frames(H, W, cls, seed=H + W)])
        tr = np.random.default_rng(H * 7 + W)
        target = np.roll(frames, (1, 2), (1, 2))                 # overlaps the mask's blobs in part
        target[tr.random(target.shape) < 0.3] = fill if fill < NCLS else 0
        target[-1] = 255                                         # an unlabelled frame
        _CACHE[key] = (frames, target) + C.largest_component_frames(frames, cls, conn, fill, target)
    return _CACHE[key]


def _counts(mask, target):
    """argmax_dice-style counts [F, NCLS, 3] with torch."""
    cs = torch.arange(NCLS, device=mask.device, dtype=torch.uint8).view(1, NCLS, 1, 1)
    a, b = mask.unsqueeze(1) == cs, target.unsqueeze(1) == cs
    return torch.stack([(a & b).sum((2, 3)), a.sum((2, 3)), b.sum((2, 3))], -1)


@pytest.mark.parametrize("F,H,W", SHAPES)
def test_largest_component_matches_the_reference(hip, F, H, W):
    for conn, cls, fill in _combos(H, W):
        frames, target, want_out, want_info = _case(F, H, W, conn, cls, fill)
        dm, dt = torch.from_numpy(frames).cuda(), torch.from_numpy(target).cuda()
        out, info = hip.largest_component(dm, cls=cls, connectivity=conn, fill=fill, target=dt)
        assert out.shape == dm.shape and out.dtype == torch.uint8 and info.shape == (frames.shape[0], 8) and info.dtype == torch.int32
        got_info = info.cpu().numpy()
        assert np.array_equal(got_info, want_info), (conn, cls, fill, np.flatnonzero((got_info != want_info).any(1)))
        assert np.array_equal(out.cpu().numpy(), want_out), (conn, cls, fill)
        assert torch.equal(dm.cpu(), torch.from_numpy(frames))                               # the input is left alone
        # without a target: the same mask, no hits
        out2, info2 = hip.largest_component(dm, cls=cls, connectivity=conn, fill=fill)
        assert torch.equal(out2, out) and torch.equal(info2[:, :4], info[:, :4]) and not info2[:, 4:].any()
        # in place equals out of place
        work = dm.clone()
        out3, info3 = hip.largest_component(work, cls=cls, connectivity=conn, fill=fill, target=dt, out=work)
        assert out3 is work and torch.equal(work, out) and torch.equal(info3, info)
        # the counts of the filtered mask from the unfiltered ones, exactly
        if fill < NCLS:
            assert torch.equal(hip.counts_after_largest(_counts(dm, dt), info, cls, fill), _counts(out, dt))


@pytest.mark.parametrize("F,H,W,offs", [(4, 30, 58, (1, 7, 15)), (2, 121, 127, (1, 15)), (6, 112, 112, (7,))])
def test_largest_component_at_any_byte_address(hip, F, H, W, offs):
    """mask, target and out as views at odd offsets into buffers: the bytes around the mask are of the class and may neither count nor connect,
    the bytes around out keep their sentinel.  out is tried at the mask's own alignment (vector stores) and at another (byte stores)."""
    conn, cls, fill = 8, 1, 3
    frames, target, want_out, want_info = _case(F, H, W, conn, cls, fill)
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
            out, info = hip.largest_component(view, cls=cls, connectivity=conn, fill=fill, target=tview, out=oview)
            assert np.array_equal(info.cpu().numpy(), want_info), (off, out_off)
            assert np.array_equal(oview.cpu().numpy(), want_out), (off, out_off)
            assert (obuf[:out_off] == 0xEE).all() and (obuf[out_off + n:] == 0xEE).all()
            assert (buf[:off] == cls).all() and (buf[off + n:] == cls).all()
        _, info = hip.largest_component(view, cls=cls, connectivity=conn, fill=fill, target=tview, out=view)      # in place at the odd address
        assert np.array_equal(view.cpu().numpy(), want_out) and np.array_equal(info.cpu().numpy(), want_info)
        assert (buf[:off] == cls).all() and (buf[off + n:] == cls).all()


@pytest.mark.parametrize("H,W", [(112, 112), (144, 160)])
def test_largest_component_is_reproducible_and_capturable(hip, H, W):
    """LDS form and workspace form: two calls agree; a captured call replays on new input (the workspace belongs to the graph's pool)."""
    a = np.concatenate([_random_frames(3, H, W, seed=11), _special_frames(H, W, 1, seed=1)[:2]])
    b = np.concatenate([_random_frames(3, H, W, seed=12), _special_frames(H, W, 1, seed=2)[:2]])
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    first, second = hip.largest_component(da, target=db), hip.largest_component(da, target=db)
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    static, static_t = da.clone(), db.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = hip.largest_component(static, cls=1, connectivity=4, fill=0, target=static_t)
    static.copy_(db); static_t.copy_(da)
    g.replay()
    torch.cuda.synchronize()
    want = hip.largest_component(db, cls=1, connectivity=4, fill=0, target=da)
    assert all(torch.equal(x, y) for x, y in zip(out, want))
    ref_out, ref_info = C.largest_component_frames(b, 1, 4, 0, a)
    assert np.array_equal(out[0].cpu().numpy(), ref_out) and np.array_equal(out[1].cpu().numpy(), ref_info)


def test_lv_measure_of_the_filtered_mask_is_the_clean_measurement(hip):
    """The feature's purpose, on the device: ellipse + island -> largest_component -> lv_measure equals lv_measure(ellipse) on every output."""
    clean = np.stack([R.ellipse_mask(112, 112, 56, 56, 40, 18, 20), R.ellipse_mask(112, 112, 56, 56, 32, 13, 20),
                      R.ellipse_mask(112, 112, 50, 60, 36, 15, 150), R.ellipse_mask(112, 112, 56, 56, 40, 18, 20)])
    dirty = clean.copy()
    for f, (cy, cx, r) in enumerate(((2, 2, 0), (12, 100, 6), (100, 15, 8), (12, 12, 4))):
        C.disc(dirty[f], cy, cx, r)
    dc, dd = torch.from_numpy(clean).cuda(), torch.from_numpy(dirty).cuda()
    moved = hip.lv_measure(dd)
    want = hip.lv_measure(dc)
    assert not torch.equal(moved[0][:, 10], want[0][:, 10])                                  # the islands do move the long axis
    for conn in (4, 8):
        out, info = hip.largest_component(dd, connectivity=conn)
        assert torch.equal(out, dc) and info[:, 0].tolist() == [2] * 4 and torch.equal(info[:, 2], want[0][:, 0].int())
        assert all(torch.equal(x, y) for x, y in zip(hip.lv_measure(out), want))
    ef = lambda m: hip.lv_ef(m[2][..., 1].reshape(2, 2).contiguous(), m[0][..., 0].reshape(2, 2).contiguous())
    assert all(torch.equal(x, y) for x, y in zip(ef(hip.lv_measure(hip.largest_component(dd)[0])), ef(want)))


def test_leading_dimensions_are_kept(hip):
    frames = _random_frames(6, 30, 58, seed=3)
    dm = torch.from_numpy(frames).cuda()
    flat_out, flat_info = hip.largest_component(dm, cls=2, connectivity=8, fill=3, target=dm)
    out, info = hip.largest_component(dm.view(2, 3, 30, 58), cls=2, connectivity=8, fill=3, target=dm.view(2, 3, 30, 58))
    assert out.shape == (2, 3, 30, 58) and info.shape == (2, 3, 8)
    assert torch.equal(out.view(6, 30, 58), flat_out) and torch.equal(info.view(6, 8), flat_info)
    one, one_info = hip.largest_component(dm[0], cls=2, connectivity=8, fill=3, target=dm[0])
    assert one.shape == (30, 58) and one_info.shape == (8,) and torch.equal(one, flat_out[0]) and torch.equal(one_info, flat_info[0])
    assert torch.equal(hip.counts_after_largest(_counts(dm, dm).view(2, 3, NCLS, 3), info, 2, 3), _counts(flat_out, dm).view(2, 3, NCLS, 3))
