"""gdkvm_overlay_native on the device against tests/overlay_reference.py, byte for byte, and its two callers in gdkvm_amd.predict against the
restatement applied to their own inputs.  The shapes sit where the kernel can go wrong rather than at the workload's size: single pixels and
rows, widths on both sides of a run and of four runs with odd h0 w0 (every frame starts at another alignment mod 16 in the inputs and mod 16
in out), class edges on every row around a band boundary, clip counts around one launch's, more items than workgroups, the bytes the rule
never draws, and every buffer in turn off the 16-byte grid with guard bytes around out."""
import os
import re

import numpy as np
import pytest
import torch

from tests import overlay_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HDR = open(os.path.join(ROOT, "include", "gdkvm.h")).read()
_define = lambda name: int(re.search(r"#define GDKVM_OVERLAY_NATIVE_" + name + r" (\d+)", _HDR).group(1))
RUN, BAND_RUNS, BAND_ROWS, MAX_WG, CLIPS = _define("RUN"), _define("BAND_RUNS"), _define("BAND_ROWS"), _define("MAX_WG"), _define("CLIPS")
ERR_SHAPE = int(re.search(r"GDKVM_ERR_SHAPE = (-?\d+)", _HDR).group(1))


def band_rows(h0, w0):
    """rows of a band, from the header's text: the most whole rows whose run slots (a head and ceil(w0 / RUN) runs per row) number at most
    BAND_RUNS, at least 1, at most BAND_ROWS (and h0)"""
    return min(max(BAND_RUNS // (1 + -(-w0 // RUN)), 1), BAND_ROWS, h0)


def _check(hip, g, m, r, sizes, T, ncls, w, alpha=96):
    """ops.overlay_native on the device copies of the flat arrays == the restatement; returns the device result"""
    pal, rpal = R.PAL[:ncls], R.REF_PAL[:ncls]
    want = R.overlay_native(g, m, r, sizes, T, ncls, w, alpha, pal, rpal)
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
    got = hip.overlay_native(dev(g), dev(m), sizes, T, ncls, reference=dev(r), width=w, alpha=alpha, palette=pal.tolist(),
                             reference_palette=rpal.tolist())
    assert got.dtype == torch.uint8 and got.is_cuda and got.numel() == want.size
    bad = np.nonzero(got.cpu().numpy() != want)[0]
    assert bad.size == 0, (sizes, T, ncls, w, alpha, r is not None, bad[:8].tolist())
    return got


def _case(seed, sizes, T, ncls):
    rng = np.random.default_rng(seed)
    m = R.pack([R.blobs(rng, T, h, wd, ncls) for h, wd in sizes])[0]
    r = R.pack([R.blobs(rng, T, h, wd, ncls) for h, wd in sizes])[0]
    return rng.integers(0, 256, m.size, dtype=np.uint8), m, r


SMALL = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 3), (17, 33), (33, 65)]


@pytest.mark.parametrize("with_ref", [False, True], ids=["no_ref", "ref"])
@pytest.mark.parametrize("w", [1, 2, 3])
@pytest.mark.parametrize("ncls", [2, 4, 8])
def test_sizes_and_parameters(hip, ncls, w, with_ref):
    """1 x 1 to 33 x 65 in one ragged batch at T = 2 (odd h0 w0: the frames start at many alignments), and every frame size alone"""
    g, m, r = _case(10 * ncls + w, SMALL, 2, ncls)
    _check(hip, g, m, r if with_ref else None, SMALL, 2, ncls, w)
    offs, _ = R.offsets(SMALL, 2)
    for b, (h0, w0) in enumerate(SMALL[:5]):
        sl = slice(offs[b], offs[b] + 2 * h0 * w0)
        _check(hip, g[sl].copy(), m[sl].copy(), r[sl].copy() if with_ref else None, [(h0, w0)], 2, ncls, w)


@pytest.mark.parametrize("alpha", [0, 1, 96, 255, 256])
def test_alpha_range(hip, alpha):
    g, m, r = _case(alpha, [(17, 33)], 2, 4)
    _check(hip, g, m, r, [(17, 33)], 2, 4, 2, alpha)


@pytest.mark.parametrize("w", [1, 3])
def test_widths_around_a_run_and_four_runs(hip, w):
    """w0 on both sides of RUN and of 4 RUN, h0 = 3 and T = 3, a 1 x 3 clip between every two: the frames of the six widths start at eleven
    of the sixteen alignments in the inputs (and, 3 being invertible mod 16, at as many in out), in one call, and each size alone"""
    edge = [(3, RUN - 1), (3, RUN), (3, RUN + 1), (3, 4 * RUN - 1), (3, 4 * RUN), (3, 4 * RUN + 1)]
    sizes = [s for e in edge for s in (e, (1, 3))]
    g, m, r = _case(20 + w, sizes, 3, 4)
    offs = R.offsets(sizes, 3)[0]
    starts = {(off + t * h0 * w0) % 16 for off, (h0, w0) in zip(offs, sizes) for t in range(3) if (h0, w0) != (1, 3)}
    assert len(starts) >= 8
    _check(hip, g, m, r, sizes, 3, 4, w)
    _check(hip, g, m, None, sizes, 3, 4, w)
    for (h0, w0), off in zip(sizes[::2], offs[::2]):
        sl = slice(off, off + 3 * h0 * w0)
        _check(hip, g[sl].copy(), m[sl].copy(), r[sl].copy(), [(h0, w0)], 3, 4, w)


def test_ragged_batch_of_larger_clips(hip):
    sizes = [(97, 130), (64, 64), (33, 17), (5, 300), (130, 97)]
    g, m, r = _case(30, sizes, 2, 4)
    _check(hip, g, m, r, sizes, 2, 4, 2)
    _check(hip, g, m, None, sizes, 2, 4, 3)


@pytest.mark.parametrize("w", [1, 2, 3])
@pytest.mark.parametrize("hw", [(100, 200), (150, 20), (11, 2048)], ids=["36_rows", "row_cap", "3_rows"])
def test_class_edges_around_a_band_boundary(hip, hw, w):
    """A frame of several bands; frame t has a horizontal class edge at row e_t, for every e from w rows above to w rows below the first band
    boundary and the second: class 1 above the edge and class 2 below in the mask, the other way round in the ref.  The contour of either
    class then lies in rows that one band owns and reads from the rows its neighbour owns."""
    h0, w0 = hw
    rpb = band_rows(h0, w0)
    assert h0 > 2 * rpb + w                                      # at least three bands, and every edge inside the frame
    assert rpb == {(100, 200): 36, (150, 20): BAND_ROWS, (11, 2048): 3}[hw]
    edges = [k * rpb + d for k in (1, 2) for d in range(-w, w + 1)]
    T = len(edges)
    rows = np.arange(h0)[None, :, None]
    e = np.asarray(edges)[:, None, None]
    m = np.broadcast_to(np.where(rows < e, 1, 2), (T, h0, w0)).astype(np.uint8)
    r = np.broadcast_to(np.where(rows < e, 2, 1), (T, h0, w0)).astype(np.uint8).copy()
    r[:, :, w0 // 2:] = 0                                        # the ref's contour also ends in the middle of a row
    rng = np.random.default_rng(40)
    g = rng.integers(0, 256, m.size, dtype=np.uint8)
    _check(hip, g, m.reshape(-1), r.reshape(-1), [hw], T, 3, w)
    # and vertical structure across the boundary: random blobs on the same geometry
    g2, m2, r2 = _case(41 + w, [hw], 2, 4)
    _check(hip, g2, m2, r2, [hw], 2, 4, w)


@pytest.mark.parametrize("clips", [CLIPS - 1, CLIPS, CLIPS + 1, 2 * CLIPS + 1])
def test_clip_counts_around_one_launch(hip, clips):
    """3 x 5 frames at T = 2 with content of their own per clip: a launch holds CLIPS clips and the next one starts at the carried offset"""
    sizes = [(3, 5)] * clips
    g, m, r = _case(50, sizes, 2, 4)
    _check(hip, g, m, r, sizes, 2, 4, 2)


def test_more_items_than_workgroups(hip):
    """CLIPS clips x 65 frames of 2 x 3: one band each, more (clip, frame, band) items than MAX_WG in the first launch"""
    T, sizes = MAX_WG // CLIPS + 1, [(2, 3)] * (CLIPS + 6)
    assert CLIPS * T > MAX_WG
    g, m, r = _case(60, sizes, T, 4)
    _check(hip, g, m, r, sizes, T, 4, 1)


def test_bytes_that_are_never_drawn(hip):
    """Both masks made of class bytes and of every kind of byte the rule does not draw: 0, ncls .. 254, 255"""
    rng = np.random.default_rng(70)
    sizes, T = [(21, 37), (8, 8)], 2
    total = R.offsets(sizes, T)[1]
    for ncls in (2, 4, 8):
        pool = np.array([0, 1, ncls - 1, ncls, ncls + 1, 8, 9, 127, 128, 129, 200, 254, 255], np.uint8)
        m, r = rng.choice(pool, total), rng.choice(pool, total)
        g = rng.integers(0, 256, total, dtype=np.uint8)
        _check(hip, g, m, r, sizes, T, ncls, 2)
        # a mask of undrawn bytes only is the grey frame in three channels
        got = hip.overlay_native(torch.from_numpy(g).cuda(), torch.from_numpy(rng.choice(pool[3:], total)).cuda(), sizes, T, ncls)
        assert np.array_equal(got.cpu().numpy(), np.repeat(g, 3))


def test_every_buffer_off_the_16_byte_grid_and_guards_around_out(hip):
    """grey, mask, ref and out in turn sliced from a larger buffer at byte offsets 1, 2 and 3 (the others aligned); out lies between two
    guards of 64 patterned bytes, which are unchanged afterwards"""
    sizes, T, ncls, w = [(5, 3), (17, 33), (3, 50)], 3, 4, 2
    g, m, r = _case(80, sizes, T, ncls)
    n = g.size
    pal, rpal = R.PAL[:ncls], R.REF_PAL[:ncls]
    want = R.overlay_native(g, m, r, sizes, T, ncls, w, 96, pal, rpal)
    guard = torch.arange(64, dtype=torch.uint8, device="cuda") * 3 + 1
    for which in ("grey", "mask", "ref", "out", "all"):
        for k in (1, 2, 3):
            def place(a, name):
                off = k if which in (name, "all") else 0
                buf = torch.zeros(a.size + 32, dtype=torch.uint8, device="cuda")
                assert buf.data_ptr() % 16 == 0
                buf[off:off + a.size] = torch.from_numpy(a).cuda()
                return buf[off:off + a.size]
            off = k if which in ("out", "all") else 0
            obuf = torch.full((64 + 16 + 3 * n + 64 + 16,), 0xA5, dtype=torch.uint8, device="cuda")
            lo = 64 + off
            obuf[lo - 64:lo] = guard
            obuf[lo + 3 * n:lo + 3 * n + 64] = guard
            out = obuf[lo:lo + 3 * n]
            assert out.data_ptr() % 16 == off
            res = hip.overlay_native(place(g, "grey"), place(m, "mask"), sizes, T, ncls, reference=place(r, "ref"), width=w, alpha=96,
                                     palette=pal.tolist(), reference_palette=rpal.tolist(), out=out)
            assert res is out and np.array_equal(out.cpu().numpy(), want), (which, k)
            assert torch.equal(obuf[lo - 64:lo], guard) and torch.equal(obuf[lo + 3 * n:lo + 3 * n + 64], guard), (which, k)
            assert (obuf[:lo - 64] == 0xA5).all() and (obuf[lo + 3 * n + 64:] == 0xA5).all()


def test_two_calls_are_equal(hip):
    sizes = [(97, 130), (33, 17)]
    g, m, r = (torch.from_numpy(a).cuda() for a in _case(90, sizes, 2, 4))
    a = hip.overlay_native(g, m, sizes, 2, 4, reference=r, width=3)
    b = hip.overlay_native(g, m, sizes, 2, 4, reference=r, width=3)
    assert torch.equal(a, b)


def test_no_clips_is_no_launch_and_bad_arguments_are_refused(hip):
    empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
    assert hip.overlay_native(empty, empty, [], 2, 4).numel() == 0
    sizes = [(8, 8)]
    g = torch.zeros(64, dtype=torch.uint8, device="cuda")
    m = torch.ones(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(hip.GdkvmError, match="sizes must be host integers"):
        hip.overlay_native(g, m, torch.tensor(sizes, device="cuda"), 1, 4)
    with pytest.raises(hip.GdkvmError, match="palette must be host values"):
        hip.overlay_native(g, m, sizes, 1, 4, palette=torch.zeros((4, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(hip.GdkvmError, match="width = 4"):
        hip.overlay_native(g, m, sizes, 1, 4, width=4)
    with pytest.raises(hip.GdkvmError, match="tensors on different devices"):
        hip.overlay_native(g, m.cpu(), sizes, 1, 4)
    big = torch.zeros(4 * 64, dtype=torch.uint8, device="cuda")
    with pytest.raises(hip.GdkvmError, match="out must not overlap mask"):
        hip.overlay_native(g, big[:64], sizes, 1, 4, out=big[63:])
    # the C entry refuses them too, before any launch: out stays as it was
    lib = hip.load()
    host = np.array(sizes, np.int32)
    pal = np.zeros((4, 3), np.uint8)
    out = torch.full((3 * 64,), 7, dtype=torch.uint8, device="cuda")
    call = lambda **kw: lib.gdkvm_overlay_native(*[{**dict(grey=g.data_ptr(), mask=m.data_ptr(), ref=None, sz=host.ctypes.data, p=pal.ctypes.data,
                                                           rp=None, o=out.data_ptr(), nb=64, ws=None, wsb=0, clips=1, T=1, ncls=4, width=2,
                                                           alpha=96, st=None), **kw}[k]
                                                   for k in ("grey", "mask", "ref", "sz", "p", "rp", "o", "nb", "ws", "wsb", "clips", "T", "ncls",
                                                             "width", "alpha", "st")])
    for kw in (dict(width=0), dict(alpha=257), dict(ncls=9), dict(nb=63), dict(ref=m.data_ptr()), dict(o=g.data_ptr()), dict(p=None), dict(T=0)):
        assert call(**kw) == ERR_SHAPE and b"overlay_native" in lib.gdkvm_last_error(), kw
    assert call(clips=0) == 0
    torch.cuda.synchronize()
    assert (out == 7).all()
    assert call() == 0                                           # and the same call with good arguments draws: class 1 everywhere is all contour or tint
    torch.cuda.synchronize()
    assert not (out == 7).all()


def _small_model(cfg):
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    torch.manual_seed(0)
    model = GDKVM(GDKVMConfig(num_classes=cfg.data.num_classes, widths=(16, 32, 64), pixel_dim=64, value_dim=32)).eval()
    with torch.no_grad():
        model.decoder.head.bias[1] += 0.05                    # random init is one class everywhere; tilt it so masks are mixed
    return model.fuse_for_inference().cuda().to(torch.bfloat16).to(memory_format=torch.channels_last)


def test_segment_native_with_overlay_is_the_restatement_of_its_own_masks(hip):
    """predict.segment_native(..., overlay=True) with the small random model of tests/test_native_input_gpu.py on three ragged clips: the
    pictures are the restatement applied to the clips and to the call's own native masks, with the configuration's overlay section; and
    overlay=False returns what it returned before, key for key."""
    from gdkvm_amd.config import load_config
    from gdkvm_amd.predict import segment_native
    cfg = load_config(None, ["data.size=64", "data.lv_fill_holes=4", "data.temporal_vote=1", "overlay.width=3", "overlay.alpha=120"])
    model = _small_model(cfg)
    rng = np.random.default_rng(5)
    sizes = [(97, 130), (64, 64), (33, 17)]
    clips = [rng.integers(0, 256, (3, h0, w0), dtype=np.uint8) for h0, w0 in sizes]
    plain = segment_native(model, cfg, [torch.from_numpy(c) for c in clips])
    assert set(plain) == {"masks", "grid_mask", "frames", "sizes", "report"}
    res = segment_native(model, cfg, [torch.from_numpy(c) for c in clips], overlay=True)
    assert set(res) == set(plain) | {"overlay"}
    assert torch.equal(res["grid_mask"], plain["grid_mask"]) and torch.equal(res["frames"], plain["frames"]) and res["sizes"] == plain["sizes"]
    assert res["report"]["per_clip"] == plain["report"]["per_clip"]
    ncls = cfg.data.num_classes
    pal = np.array(hip.OVERLAY_PALETTE[:ncls], np.uint8)
    drawn = 0
    for b, (h0, w0) in enumerate(sizes):
        assert torch.equal(res["masks"][b], plain["masks"][b])
        pic, msk = res["overlay"][b], res["masks"][b].cpu().numpy()
        assert pic.dtype == torch.uint8 and pic.is_cuda and tuple(pic.shape) == (3, h0, w0, 3)
        for t in range(3):
            want = R.overlay_frame(clips[b][t], msk[t], None, ncls, 3, 120, pal, pal)
            assert np.array_equal(pic[t].cpu().numpy(), want), (b, t)
        drawn += int(R.class_bytes(msk, ncls).sum())
    assert drawn > 0                                             # the masks are mixed: something was drawn


def test_overlay_clip_of_a_dataset_clip_with_its_labels_as_reference(hip):
    from gdkvm_amd.config import load_config
    from gdkvm_amd.data import SyntheticEchoClips
    from gdkvm_amd.predict import overlay_clip
    cfg = load_config(None, ["data.size=48", "data.frames=3", "overlay.palette=[[0,0,0],[250,10,20],[30,240,40],[50,60,230]]"])
    ds = SyntheticEchoClips(2, 3, 48, num_classes=cfg.data.num_classes, as_uint8=True)
    frames, labels = ds[1]
    grey = frames[:, 0].contiguous()
    mask = torch.roll(labels, shifts=(2, -3), dims=(1, 2)).cuda()        # a "prediction" that is the tracing moved: both contours show
    pic = overlay_clip(grey, mask, cfg, reference=labels)
    assert pic.is_cuda and pic.dtype == torch.uint8 and tuple(pic.shape) == (3, 48, 48, 3)
    pal = np.array(cfg.overlay.palette, np.uint8)
    rpal = np.array(hip.OVERLAY_REFERENCE_PALETTE[:4], np.uint8)
    for t in range(3):
        want = R.overlay_frame(grey[t].numpy(), mask[t].cpu().numpy(), labels[t].numpy(), 4, cfg.overlay.width, cfg.overlay.alpha, pal, rpal)
        assert np.array_equal(pic[t].cpu().numpy(), want), t
    shown = pic.cpu().numpy().reshape(-1, 3)
    assert (shown == rpal[1]).all(1).any() and (shown == pal[1]).all(1).any()
    # without a reference, on the same mask
    pic2 = overlay_clip(grey, mask, cfg)
    want = R.overlay_frame(grey[0].numpy(), mask[0].cpu().numpy(), None, 4, cfg.overlay.width, cfg.overlay.alpha, pal, rpal)
    assert np.array_equal(pic2[0].cpu().numpy(), want)
    with pytest.raises(hip.GdkvmError, match="overlay_clip: frames_u8, mask and reference must be uint8"):
        overlay_clip(grey[:2], mask, cfg)
