"""Overlays at native size without a device: tests/overlay_reference.py (the rule of gdkvm_overlay_native in include/gdkvm.h) against scipy's
iterated erosion and against the surface of tests/surface_reference.py, the precedence and the rounding by hand, the rule's identities,
ops.overlay_native's host path and refusals, the C entry's refusals, and the configuration keys."""
import os

import numpy as np
import pytest
import torch

from tests import overlay_reference as R
from tests import surface_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_contour_is_the_class_minus_its_iterated_erosion():
    """200 random and median-filtered masks with 255 sprinkled in, ncls 2..8, w 1..3: per class, contour == X & ~erode^w(X), the outside of
    the frame being background; nothing but class bytes is ever a contour pixel."""
    from scipy import ndimage as ndi                                     # (no skip: this is the restatement's one independent check)
    rng = np.random.default_rng(0)
    for trial in range(200):
        h, wd = (int(v) for v in rng.integers(1, 40, 2))
        ncls, w = int(rng.integers(2, 9)), int(rng.integers(1, 4))
        m = rng.integers(0, ncls, (h, wd)).astype(np.uint8)
        if trial % 2:
            m = ndi.median_filter(m, 5)
        m[rng.random((h, wd)) < 0.02] = 255
        c = R.contour(m, ncls, w)
        for k in range(1, ncls):
            X = m == k
            er = ndi.binary_erosion(X, iterations=w, border_value=0) if X.any() else X
            assert np.array_equal(c & X, X & ~er), (trial, k)
        assert not c[(m == 0) | (m >= ncls)].any()


def test_width_one_is_the_surface_of_the_surface_distances():
    rng = np.random.default_rng(1)
    for h, wd in ((1, 1), (1, 9), (9, 1), (12, 17), (31, 30)):
        for ncls in (2, 4, 8):
            m = R.blobs(rng, 1, h, wd, ncls)[0]
            c = R.contour(m, ncls, 1)
            for k in range(1, ncls):
                assert np.array_equal(c & (m == k), S.surface(m == k)), (h, wd, ncls, k)


def test_precedence_and_rounding_by_hand():
    """5 x 5, ncls 3, w 1, alpha 96, g = 3 everywhere, pal[1] = (7, 12, 20).
    mask: a 3 x 3 block of class 1 in the middle -- its ring of 8 is contour, its centre pixel is interior.
    ref:  class 2 on the whole frame -- its contour is the frame's border ring of 16, the 3 x 3 inside is interior.
    So the ring of the block shows pal[1] (case 1), the border ring ref_pal[2] (case 2: the mask holds 0 there), the centre pixel the tint
    (case 3), and without the ref the border ring is grey (case 4).  The tint of the red channel is (3 * 160 + 7 * 96 + 128) >> 8 with
    3 * 160 + 7 * 96 = 1152 = 4.5 * 256 exactly: the half rounds UP, to 5.  Green: 480 + 1152 = 6.375 * 256 -> 6.  Blue: 480 + 1920 =
    9.375 * 256 -> 9."""
    pal = np.array([[0, 0, 0], [7, 12, 20], [1, 1, 1]], np.uint8)
    rpal = np.array([[0, 0, 0], [90, 91, 92], [200, 201, 202]], np.uint8)
    g = np.full((5, 5), 3, np.uint8)
    m = np.zeros((5, 5), np.uint8)
    m[1:4, 1:4] = 1
    r = np.full((5, 5), 2, np.uint8)
    ring = np.zeros((5, 5), bool)
    ring[1:4, 1:4] = True
    ring[2, 2] = False
    border = np.ones((5, 5), bool)
    border[1:4, 1:4] = False
    assert np.array_equal(R.contour(m, 3, 1), ring) and np.array_equal(R.contour(r, 3, 1), border)
    assert (3 * 160 + 7 * 96) % 256 == 128                               # exactly .5
    out = R.overlay_frame(g, m, r, 3, 1, 96, pal, rpal)
    assert (out[ring] == pal[1]).all()                                   # case 1 (over the mask's own tint: 1 > 3)
    assert (out[border] == rpal[2]).all()                                # case 2 over grey: 2 > 4
    assert out[2, 2].tolist() == [5, 6, 9]                               # case 3, rounded half up
    # 1 > 2: a ref whose contour lies on the mask's ring does not show there; 2 > 3: where it lies on the mask's interior it does
    r2 = np.zeros((5, 5), np.uint8)
    r2[2, 1:3] = 1                                                       # two pixels, both contour: (2, 1) on the ring, (2, 2) on the centre
    out2 = R.overlay_frame(g, m, r2, 3, 1, 96, pal, rpal)
    assert out2[2, 1].tolist() == pal[1].tolist() and out2[2, 2].tolist() == rpal[1].tolist()
    # case 4: without a ref the border ring is the grey value in three channels, and the rest is as before
    out3 = R.overlay_frame(g, m, None, 3, 1, 96, pal, rpal)
    assert (out3[border] == 3).all() and (out3[ring] == pal[1]).all() and out3[2, 2].tolist() == [5, 6, 9]


def test_identities():
    rng = np.random.default_rng(2)
    for ncls in (2, 4, 8):
        for w in (1, 2, 3):
            g = rng.integers(0, 256, (19, 23)).astype(np.uint8)
            m = R.blobs(rng, 1, 19, 23, ncls)[0]
            grey3 = np.repeat(g[..., None], 3, -1)
            pal, rpal = R.PAL[:ncls], R.REF_PAL[:ncls]
            # a mask without class bytes returns the grey frame in three channels
            for empty in (np.zeros_like(m), np.full_like(m, 255), np.full_like(m, ncls)):
                assert np.array_equal(R.overlay_frame(g, empty, None, ncls, w, 96, pal, rpal), grey3)
            pc, lab = R.contour(m, ncls, w), R.class_bytes(m, ncls)
            # alpha = 0 draws contours only
            o0 = R.overlay_frame(g, m, None, ncls, w, 0, pal, rpal)
            assert np.array_equal(o0[~pc], grey3[~pc]) and np.array_equal(o0[pc], pal[m[pc]])
            # alpha = 256 paints the class solid
            o1 = R.overlay_frame(g, m, None, ncls, w, 256, pal, rpal)
            assert np.array_equal(o1[lab], pal[m[lab]]) and np.array_equal(o1[~lab], grey3[~lab])
            # wider contours contain narrower ones
            if w > 1:
                assert not (R.contour(m, ncls, w - 1) & ~pc).any()


def _ragged(rng, sizes, T, ncls):
    m = R.pack([R.blobs(rng, T, h, wd, ncls) for h, wd in sizes])[0]
    r = R.pack([R.blobs(rng, T, h, wd, ncls) for h, wd in sizes])[0]
    return rng.integers(0, 256, m.size, dtype=np.uint8), m, r


def test_ops_host_path_equals_the_restatement():
    from gdkvm_amd import ops
    rng = np.random.default_rng(3)
    sizes, T = [(40, 65), (3, 15), (9, 7)], 2
    for ncls, w, alpha in ((2, 1, 0), (4, 2, 96), (8, 3, 256), (4, 3, 1)):
        g, m, r = _ragged(rng, sizes, T, ncls)
        pal, rpal = R.PAL[:ncls], R.REF_PAL[:ncls]
        for ref in (None, r):
            want = R.overlay_native(g, m, ref, sizes, T, ncls, w, alpha, pal, rpal)
            for sz, p in ((sizes, pal.tolist()), (torch.tensor(sizes, dtype=torch.int32), torch.from_numpy(pal.copy()))):
                got = ops.overlay_native(torch.from_numpy(g), torch.from_numpy(m), sz, T, ncls, reference=None if ref is None else torch.from_numpy(ref),
                                         width=w, alpha=alpha, palette=p, reference_palette=rpal.tolist())
                assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want), (ncls, w, alpha)
        for b, (h0, w0) in enumerate(sizes):
            v = ops.native_rgb_frames(got, sizes, T, b)
            assert tuple(v.shape) == (T, h0, w0, 3)
            lo = R.offsets(sizes, T)[0][b]
            assert np.array_equal(v.numpy().reshape(-1), want[3 * lo:3 * (lo + T * h0 * w0)])
    # the defaults: eight colours each, class 0 aside all different, the reference's near white
    assert len(ops.OVERLAY_PALETTE) == len(ops.OVERLAY_REFERENCE_PALETTE) == 8
    assert len(set(ops.OVERLAY_PALETTE[1:])) == 7 and all(max(c) >= 220 and min(c) <= 128 for c in ops.OVERLAY_PALETTE[1:])
    assert all(min(c) >= 190 for c in ops.OVERLAY_REFERENCE_PALETTE[1:])
    g, m, r = _ragged(rng, sizes, T, 4)
    got = ops.overlay_native(torch.from_numpy(g), torch.from_numpy(m), sizes, T, 4, reference=torch.from_numpy(r))
    want = R.overlay_native(g, m, r, sizes, T, 4, 2, 96, np.array(ops.OVERLAY_PALETTE[:4], np.uint8), np.array(ops.OVERLAY_REFERENCE_PALETTE[:4], np.uint8))
    assert np.array_equal(got.numpy(), want)
    # out=: written in place and returned
    buf = torch.zeros(3 * g.size + 5, dtype=torch.uint8)
    assert ops.overlay_native(torch.from_numpy(g), torch.from_numpy(m), sizes, T, 4, reference=torch.from_numpy(r), out=buf) is buf
    assert np.array_equal(buf[:3 * g.size].numpy(), want) and not buf[3 * g.size:].any()
    assert {"gdkvm_overlay_native", "gdkvm_overlay_native_workspace_bytes"} <= set(ops.SIGNATURES)


def test_ops_refusals_without_a_device():
    from gdkvm_amd import ops
    sizes, T = [(5, 6), (7, 3)], 2
    total = T * (30 + 21)
    g, m = torch.zeros(total, dtype=torch.uint8), torch.zeros(total, dtype=torch.uint8)
    shared = torch.zeros(4 * total, dtype=torch.uint8)
    pal4 = [[1, 2, 3]] * 4
    bad = [(dict(sizes=torch.ones((2, 2), dtype=torch.int32, device="meta")), "sizes must be host integers"),
           (dict(palette=torch.ones((4, 3), dtype=torch.uint8, device="meta")), "palette must be host values"),
           (dict(reference_palette=torch.ones((4, 3), dtype=torch.uint8, device="meta")), "reference_palette must be host values"),
           (dict(width=0), "width = 0 must be an integer in 1..3"), (dict(width=4), "width = 4"), (dict(width=True), "width = True"),
           (dict(alpha=257), "alpha = 257 must be an integer in 0..256"), (dict(alpha=-1), "alpha = -1"), (dict(alpha=96.0), "alpha = 96.0"),
           (dict(grey=g[:-1]), f"grey must be a flat uint8 tensor of at least {total}"), (dict(mask=m[:-1]), "mask must be a flat uint8"),
           (dict(reference=m[:-1]), "reference must be a flat uint8"), (dict(mask=m.to(torch.int32)), "mask must be a flat uint8"),
           (dict(out=torch.zeros(3 * total - 1, dtype=torch.uint8)), f"out must be a flat uint8 tensor of at least {3 * total}"),
           (dict(palette=pal4[:3]), "palette has 3 colours for 4 classes"), (dict(reference_palette=pal4 + pal4), "reference_palette has 8 colours"),
           (dict(palette=[[1, 2, 3]] * 3 + [[1, 2, 256]]), r"palette\[3\] = \(1, 2, 256\) is no \(r, g, b\)"),
           (dict(palette=[[1, 2, 3]] * 3 + [[1, 2]]), r"palette\[3\]"), (dict(palette=torch.ones((4, 3))), "palette must hold integers"),
           (dict(grey=shared[:total], out=shared[total - 1:]), "out must not overlap grey"),
           (dict(mask=shared[3 * total:], out=shared[2:3 * total + 2]), "out must not overlap mask"),
           (dict(reference=shared[3 * total:], out=shared[1:3 * total + 1]), "out must not overlap reference"),
           (dict(num_classes=1), "num_classes = 1"), (dict(num_classes=9), "num_classes = 9"), (dict(T=0), "T = 0"),
           (dict(sizes=[(5, 6), (0, 3)]), r"sizes\[1\] = 0 x 3 outside 1..2048"), (dict(sizes=[(5, 6), (7, 2049)]), "outside 1..2048")]
    for kw, msg in bad:
        args = {"grey": g, "mask": m, "sizes": sizes, "T": T, "num_classes": 4, **kw}
        with pytest.raises(ops.GdkvmError, match="overlay_native: .*" + msg):
            ops.overlay_native(**args)
    with pytest.raises(ops.GdkvmError, match="native_rgb_frames: clip 2 is none of the 2 clips"):
        ops.native_rgb_frames(shared, sizes, T, 2)
    with pytest.raises(ops.GdkvmError, match=f"native_rgb_frames: flat must be a 1-D tensor of at least {3 * total}"):
        ops.native_rgb_frames(shared[:3 * total - 1], sizes, T, 0)
    assert ops.overlay_native(g[:0], m[:0], [], T, 4).numel() == 0           # no clips: nothing to draw


def test_entry_refuses_bad_arguments_without_a_device():
    """The C entry validates everything before its first device call, so it answers on a machine without a GPU too."""
    from gdkvm_amd import ops
    lib = ops.load()
    sizes = np.array([[5, 6], [7, 3]], np.int32)
    total = 2 * (30 + 21)
    g, m, r = np.zeros(total + 16, np.uint8), np.zeros(total + 16, np.uint8), np.zeros(total + 16, np.uint8)
    out = np.zeros(3 * total + 16, np.uint8)
    pal, rpal = np.zeros((4, 3), np.uint8), np.zeros((4, 3), np.uint8)

    def call(grey=g.ctypes.data, mask=m.ctypes.data, ref=r.ctypes.data, sz=sizes, p=pal.ctypes.data, rp=rpal.ctypes.data, o=out.ctypes.data,
             nb=total, clips=2, T=2, ncls=4, width=2, alpha=96):
        return lib.gdkvm_overlay_native(grey, mask, ref, sz.ctypes.data if sz is not None else None, p, rp, o, nb, None, 0, clips, T, ncls,
                                        width, alpha, None)

    cases = [dict(clips=-1), dict(T=0), dict(ncls=1), dict(ncls=9), dict(width=0), dict(width=4), dict(alpha=-1), dict(alpha=257),
             dict(sz=np.array([[5, 6], [0, 3]], np.int32)), dict(sz=np.array([[5, 6], [7, 2049]], np.int32)), dict(grey=None), dict(mask=None),
             dict(sz=None), dict(p=None), dict(o=None), dict(rp=None), dict(nb=total - 1), dict(o=g.ctypes.data), dict(o=m.ctypes.data + 5),
             dict(o=r.ctypes.data - 3 * total + 1), dict(grey=out.ctypes.data + 3 * total - 1)]
    for kw in cases:
        assert call(**kw) == -1, kw
        assert b"overlay_native" in lib.gdkvm_last_error(), kw
    assert call(clips=0) == 0
    assert call(clips=0, grey=None, mask=None, sz=None, p=None, o=None) == 0
    assert lib.gdkvm_overlay_native_workspace_bytes(16, 10, 4, 2) == 0


def test_geometry_constants_are_mirrored():
    import re
    from gdkvm_amd import ops
    hdr = open(os.path.join(ROOT, "include", "gdkvm.h")).read()
    for name in ("RUN", "BAND_RUNS", "BAND_ROWS", "MAX_WG", "CLIPS"):
        assert int(re.search(r"#define GDKVM_OVERLAY_NATIVE_" + name + r" (\d+)", hdr).group(1)) == getattr(ops, "OVERLAY_NATIVE_" + name)


def test_overlay_config_keys():
    from gdkvm_amd.config import load_config
    path = os.path.join(ROOT, "config", "config_gdkvm_01.yaml")
    for cfg in (load_config(path), load_config(None, [])):
        o = cfg.overlay
        assert (o.alpha, o.width, o.palette, o.reference_palette) == (96, 2, None, None) and cfg.eval_stage.vis_overlay is False
    cfg = load_config(path, ["overlay.alpha=0", "overlay.width=3", "eval_stage.vis_overlay=true", "data.num_classes=2",
                             "overlay.palette=[[0,0,0],[255,0,0]]", "overlay.reference_palette=[[0,0,0],[250,250,250]]"])
    assert cfg.overlay.alpha == 0 and cfg.overlay.width == 3 and cfg.eval_stage.vis_overlay is True
    assert cfg.overlay.palette == [[0, 0, 0], [255, 0, 0]] and cfg.overlay.reference_palette == [[0, 0, 0], [250, 250, 250]]
    assert load_config(path, ["overlay.alpha=256"]).overlay.alpha == 256
    for bad, key in (("overlay.alpha=257", "overlay.alpha"), ("overlay.alpha=-1", "overlay.alpha"), ("overlay.alpha=0.5", "overlay.alpha"),
                     ("overlay.alpha=true", "overlay.alpha"), ("overlay.width=0", "overlay.width"), ("overlay.width=4", "overlay.width"),
                     ("overlay.width=two", "overlay.width"), ("eval_stage.vis_overlay=1", "eval_stage.vis_overlay"),
                     ("overlay.palette=[[0,0,0],[255,0,0]]", "overlay.palette has 2 colours, data.num_classes = 4"),
                     ("overlay.reference_palette=[[0,0,0]]", "overlay.reference_palette has 1 colours"),
                     ("overlay.palette=[[0,0,0],[1,2,3],[4,5,6],[7,8,256]]", "overlay.palette"),
                     ("overlay.palette=[[0,0,0],[1,2,3],[4,5,6],[7,8]]", "overlay.palette"), ("overlay.palette=red", "overlay.palette")):
        with pytest.raises(ValueError, match=key):
            load_config(path, [bad])
    with pytest.raises(KeyError, match="colour"):
        load_config(path, ["overlay.colour=1"])
