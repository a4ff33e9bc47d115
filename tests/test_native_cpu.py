"""Native-resolution evaluation without a device: tests/native_reference.py (the rule of gdkvm_mask_to_native in include/gdkvm.h) against
F.interpolate on float64 one-hot planes, its fixed points, ops.mask_to_native's host path and refusals, the converter's --native-masks, the
datasets' native targets, and the round trip that motivates the rule."""
import filecmp
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests import native_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# (H, W, h0, w0): up-scales, down-scales, squeezes, 1 x 1 on either side
SHAPES = [(7, 5, 11, 13), (16, 12, 5, 7), (16, 16, 23, 37), (1, 1, 4, 4), (4, 4, 1, 1), (8, 8, 8, 8), (8, 8, 16, 16), (8, 8, 24, 24),
          (6, 10, 9, 15), (12, 12, 18, 18)]


def test_rule_against_interpolate_outside_exact_ties():
    """Every pixel where the restatement and argmax(F.interpolate(one-hot float64)) disagree is an exact tie of the integer votes."""
    rng = np.random.default_rng(0)
    ties_by_shape = {}
    for shape in SHAPES:
        H, W, h0, w0 = shape
        ties_by_shape[shape] = 0
        for ncls in (2, 4, 8):
            m = rng.integers(0, ncls, (H, W)).astype(np.uint8)
            out, votes, tie = R.resize_labels(m, h0, w0, ncls)
            oh = torch.stack([torch.from_numpy((m == c).astype(np.float64)) for c in range(ncls)])[None]
            ref = TF.interpolate(oh, size=(h0, w0), mode="bilinear", align_corners=False)[0].argmax(0).numpy()
            assert not ((ref != out) & ~tie).any(), shape
            assert (votes.sum(0) == 4 * h0 * w0).all()        # the vote sums are constant per frame
            if (H, W) == (h0, w0):
                assert np.array_equal(out, m) and not tie.any()
            ties_by_shape[shape] += int(tie.sum())
    assert any(v > 0 for v in ties_by_shape.values()) and any(v == 0 for v in ties_by_shape.values())


def test_unlabelled_source_bytes_do_not_vote():
    m = np.array([[255, 255, 1], [255, 255, 1], [0, 0, 1]], np.uint8)
    out, votes, _ = R.resize_labels(m, 6, 6, 2)
    assert (out[:3, :3] == 255).all()                         # an all-255 neighbourhood: no class has a vote
    assert (votes[:, :3, :3] == 0).all() and (out[:, 5] == 1).all() and out[5, 0] == 0
    assert set(np.unique(out)) <= {0, 1, 255}
    # a byte >= ncls is as silent as 255
    assert np.array_equal(R.resize_labels(np.where(m == 255, 2, m).astype(np.uint8), 6, 6, 2)[0], out)


def test_tie_rule_by_hand():
    """2 x 2 -> 3 x 3: the centre pixel sees all four source pixels with the weight 9 each."""
    out, votes, tie = R.resize_labels(np.array([[1, 0], [0, 1]], np.uint8), 3, 3, 2)
    assert votes[:, 1, 1].tolist() == [18, 18] and tie[1, 1] and out[1, 1] == 0           # a tie goes to the smallest class
    assert out[0, 0] == 1 and out[0, 2] == 0 and out[2, 0] == 0 and out[2, 2] == 1         # the corners are their source pixel
    assert votes[:, 0, 1].tolist() == [18, 18] and out[0, 1] == 0                          # (the edge centres tie too)
    out3, votes3, _ = R.resize_labels(np.array([[2, 1], [1, 3]], np.uint8), 3, 3, 4)
    assert votes3[:, 1, 1].tolist() == [0, 18, 9, 9] and out3[1, 1] == 1
    out4, _, tie4 = R.resize_labels(np.array([[3, 2], [255, 255]], np.uint8), 3, 3, 4)
    assert tie4[1, 1] and out4[1, 1] == 2 and (out4[2] == 255).all()


def _case(rng, clips, T, H, W, ncls, sizes):
    m = rng.integers(0, ncls, (clips, T, H, W)).astype(np.uint8)
    m[rng.random(m.shape) < 0.1] = 255
    total = R.offsets(sizes, T)[1]
    g = rng.integers(0, ncls, total).astype(np.uint8)
    g[rng.random(total) < 0.2] = 255
    return m, g


def test_ops_host_path_equals_the_restatement():
    from gdkvm_amd import ops
    rng = np.random.default_rng(1)
    sizes = [(40, 65), (3, 15), (9, 7), (1, 1)]
    for ncls in (2, 4, 8):
        m, g = _case(rng, 4, 2, 9, 7, ncls, sizes)
        ref_out, ref_counts = R.mask_to_native(m, sizes, ncls, g)
        for sz in (sizes, torch.tensor(sizes, dtype=torch.int32), torch.tensor(sizes, dtype=torch.int64)):
            out, counts, offs = ops.mask_to_native(torch.from_numpy(m), sz, ncls, target=torch.from_numpy(g))
            assert np.array_equal(out.numpy(), ref_out) and counts.dtype == torch.int32 and np.array_equal(counts.numpy(), ref_counts)
            assert offs == R.offsets(sizes, 2)[0]
        out, counts, _ = ops.mask_to_native(torch.from_numpy(m), sizes, ncls)
        assert counts is None and np.array_equal(out.numpy(), ref_out)
        out, counts, _ = ops.mask_to_native(torch.from_numpy(m), sizes, ncls, target=torch.from_numpy(g), want_out=False)
        assert out is None and np.array_equal(counts.numpy(), ref_counts)
        one = ops.mask_to_native(torch.from_numpy(m[2]), [sizes[2]], ncls)[0]                 # a 3-D mask is one clip
        assert np.array_equal(one.numpy(), ops.native_frames(torch.from_numpy(ref_out), sizes, 2, 2).reshape(-1).numpy())
    flat, sz = ops.pack_native([torch.from_numpy(np.asarray(ops.native_frames(torch.from_numpy(ref_out), sizes, 2, b))) for b in range(4)])
    assert sz == sizes and np.array_equal(flat.numpy(), ref_out)
    assert ops.native_frames(flat, sizes, 2, 1).shape == (2, 3, 15)
    assert "gdkvm_mask_to_native" in ops.SIGNATURES and "gdkvm_mask_to_native_workspace_bytes" in ops.SIGNATURES


def test_ops_refusals_without_a_device():
    from gdkvm_amd import ops
    m = torch.zeros((2, 2, 4, 4), dtype=torch.uint8)
    sizes = [(5, 6), (7, 3)]
    total = 2 * (30 + 21)
    g = torch.zeros(total, dtype=torch.uint8)
    bad = [(dict(mask=m.to(torch.int32)), "mask must be uint8"), (dict(mask=m[0, 0]), "mask must be uint8"),
           (dict(mask=torch.zeros((1, 1, 4, 1025), dtype=torch.uint8), sizes=[(4, 4)]), "outside 1..1024"),
           (dict(num_classes=1), "num_classes = 1 must be an integer in 2..8"), (dict(num_classes=9), "num_classes = 9"),
           (dict(num_classes=True), "num_classes = True"), (dict(mask=torch.zeros((2, 0, 4, 4), dtype=torch.uint8)), "T = 0 frames"),
           (dict(sizes=[(5, 6)]), "1 sizes for 2 clips"), (dict(sizes=[(5, 6), (0, 3)]), r"sizes\[1\] = 0 x 3 outside 1..2048"),
           (dict(sizes=[(5, 6), (7, 2049)]), "outside 1..2048"), (dict(sizes=[(5, 6), (7.0, 3)]), "no pair of integers"),
           (dict(sizes=[(5, 6), (7, 3, 1)]), "no pair of integers"), (dict(sizes=5), "sizes must be a sequence"),
           (dict(sizes=torch.zeros((2, 3), dtype=torch.int32)), r"integer tensor \[clips, 2\]"),
           (dict(sizes=torch.ones((2, 2))), r"integer tensor \[clips, 2\]"),
           (dict(sizes=torch.ones((2, 2), dtype=torch.int32, device="meta")), "sizes must be host integers"),
           (dict(want_out=False), "neither out .* nor a target"), (dict(target=g[:-1]), f"target must be a flat uint8 tensor of at least {total}"),
           (dict(target=g.to(torch.int32)), "target must be a flat uint8"), (dict(target=g.reshape(2, -1)), "target must be a flat uint8"),
           (dict(out=g[:-1]), "out must be a flat uint8"), (dict(out=g, target=g.clone(), want_out=False), "an out tensor with want_out=False")]
    for kw, msg in bad:
        args = {"mask": m, "sizes": sizes, "num_classes": 4, **kw}
        with pytest.raises(ops.GdkvmError, match="mask_to_native: .*" + msg):
            ops.mask_to_native(**args)
    with pytest.raises(ops.GdkvmError, match="native_frames: clip 2 is none of the 2 clips"):
        ops.native_frames(g, sizes, 2, 2)
    with pytest.raises(ops.GdkvmError, match="native_frames: flat must be a 1-D tensor of at least"):
        ops.native_frames(g[:-1], sizes, 2, 0)
    with pytest.raises(ops.GdkvmError, match="pack_native: clip 1 must be uint8"):
        ops.pack_native([torch.zeros((2, 3, 3), dtype=torch.uint8), torch.zeros((3, 3, 3), dtype=torch.uint8)])
    with pytest.raises(ops.GdkvmError, match="pack_native: no clips"):
        ops.pack_native([])


def test_entry_refuses_bad_arguments_without_a_device():
    """The C entry validates everything before its first device call, so it answers on a machine without a GPU too."""
    from gdkvm_amd import ops
    lib = ops.load()
    m = np.zeros((2, 2, 4, 4), np.uint8)
    sizes = np.array([[5, 6], [7, 3]], np.int32)
    total = 2 * (30 + 21)
    out, tgt = np.zeros(total + 16, np.uint8), np.zeros(total + 16, np.uint8)
    cb = np.zeros(2 * 2 * 4 * 3 + 8, np.int32)
    c_al = cb.ctypes.data + (-cb.ctypes.data) % 16

    def call(mask=m.ctypes.data, sz=sizes, target=tgt.ctypes.data, o=out.ctypes.data, counts=c_al, nb=total, clips=2, T=2, H=4, W=4, ncls=4):
        return lib.gdkvm_mask_to_native(mask, sz.ctypes.data if sz is not None else None, target, o, counts, nb, None, 0, clips, T, H, W, ncls, None)

    cases = [dict(clips=-1), dict(T=0), dict(H=0), dict(W=1025), dict(ncls=1), dict(ncls=9), dict(sz=np.array([[5, 6], [0, 3]], np.int32)),
             dict(sz=np.array([[5, 6], [7, 2049]], np.int32)), dict(mask=None), dict(sz=None), dict(counts=None), dict(counts=c_al + 4),
             dict(o=None, target=None), dict(nb=total - 1), dict(o=m.ctypes.data), dict(o=tgt.ctypes.data + 5)]
    for kw in cases:
        assert call(**kw) == -1, kw
        assert b"mask_to_native" in lib.gdkvm_last_error(), kw
    assert call(clips=0) == 0
    assert lib.gdkvm_mask_to_native_workspace_bytes(16, 10, 256, 256, 4) == 0


def _tiny_camus(src, rng):
    from convert_camus import write_nifti
    for pid, (w, h, f) in (("patient0001", (13, 17, 6)), ("patient0002", (20, 11, 3))):
        os.makedirs(os.path.join(src, pid))
        for view in ("2CH", "4CH"):
            write_nifti(os.path.join(src, pid, f"{pid}_{view}_half_sequence.nii.gz"), rng.integers(0, 255, (w, h, f)).astype(np.uint8), (0.3, 0.2))
            write_nifti(os.path.join(src, pid, f"{pid}_{view}_half_sequence_gt.nii.gz"), rng.integers(0, 4, (w, h, f)).astype(np.uint8), (0.3, 0.2))


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_converter_native_masks_and_datasets(tmp_path):
    from PIL import Image
    from convert_camus import convert, read_nifti
    from gdkvm_amd.data import CamusPng, NpzClips, native_target_table
    src, plain, nat = str(tmp_path / "src"), str(tmp_path / "plain"), str(tmp_path / "nat")
    _tiny_camus(src, np.random.default_rng(3))
    quiet = lambda *a: None
    convert(src, plain, size=8, frames=4, split="val", log=quiet)
    convert(src, nat, size=8, frames=4, split="val", log=quiet, native_masks=True)
    # the tree without the flag is unchanged file for file, and the flag only adds files
    assert not any("native_mask" in f for f in _tree(plain))
    extra = [f for f in _tree(nat) if "native_mask" in f]
    assert sorted(set(_tree(nat)) - set(extra)) == _tree(plain) and len(extra) == 2 * (4 + 3)          # per view: 4 picked of 6 frames, 3 of 3
    assert all(filecmp.cmp(os.path.join(plain, f), os.path.join(nat, f), shallow=False) for f in _tree(plain))
    # the native PNGs are the stored labels, transposed to rows = y
    lab = read_nifti(os.path.join(src, "patient0001", "patient0001_2CH_half_sequence_gt.nii.gz"))
    pick = np.round(np.linspace(0, 5, 4)).astype(int)
    for j, f in enumerate(pick):
        got = np.asarray(Image.open(os.path.join(nat, "val", "patient0001", "2CH", f"native_mask_{j:03d}.png")))
        assert got.dtype == np.uint8 and np.array_equal(got, np.asarray(lab[:, :, f]).T)
    # CamusPng: the same frame pick as __getitem__; a frame without a file is 255; None without native masks
    ds = CamusPng(nat, "val", 4, as_uint8=True)
    assert [ds.native_hw(i) for i in range(4)] == [(17, 13), (17, 13), (11, 20), (11, 20)]
    t0 = ds.native_target(0)
    assert t0.dtype == torch.uint8 and tuple(t0.shape) == (4, 17, 13)
    assert all(np.array_equal(t0[j].numpy(), np.asarray(lab[:, :, f]).T) for j, f in enumerate(pick))
    t2 = ds.native_target(2)                                  # 3 frames on disk, T = 4: the last repeats, as in __getitem__
    assert tuple(t2.shape) == (4, 11, 20) and torch.equal(t2[3], t2[2])
    ds2 = CamusPng(nat, "val", 2, as_uint8=True)              # 4 frames on disk, T = 2: the first and the last
    assert torch.equal(ds2.native_target(0), t0[[0, 3]])
    os.remove(os.path.join(nat, "val", "patient0001", "2CH", "native_mask_001.png"))
    assert (ds.native_target(0)[1] == 255).all() and torch.equal(ds.native_target(0)[2], t0[2])
    assert native_target_table(ds).tolist() == [[17, 13], [17, 13], [11, 20], [11, 20]] and native_target_table(ds).dtype == torch.int32
    dp = CamusPng(plain, "val", 4, as_uint8=True)
    assert dp.native_hw(0) is None and dp.native_target(0) is None and native_target_table(dp) is None
    # NpzClips: an optional native_target array, as spacing_um is
    root = tmp_path / "npz" / "val"
    os.makedirs(root)
    fr, mk = np.zeros((3, 8, 8), np.uint8), np.zeros((3, 8, 8), np.uint8)
    ntv = np.random.default_rng(4).integers(0, 3, (3, 5, 9)).astype(np.uint8)
    np.savez(root / "a.npz", frames=fr, masks=mk, native_target=ntv)
    np.savez(root / "b.npz", frames=fr, masks=mk, native_target=np.zeros((4, 7, 2), np.uint8))
    dn = NpzClips(str(tmp_path / "npz"), "val", 3, as_uint8=True)
    assert dn.native_hw(0) == (5, 9) and np.array_equal(dn.native_target(0).numpy(), ntv) and tuple(dn.native_target(1).shape) == (3, 7, 2)
    assert native_target_table(dn).tolist() == [[5, 9], [7, 2]]
    np.savez(root / "c.npz", frames=fr, masks=mk)
    dn = NpzClips(str(tmp_path / "npz"), "val", 3, as_uint8=True)
    assert dn.native_target(2) is None and dn.native_hw(2) is None and native_target_table(dn) is None
    assert native_target_table(object()) is None


def test_native_eval_config_key():
    from gdkvm_amd.config import load_config
    path = os.path.join(ROOT, "config", "config_gdkvm_01.yaml")
    assert load_config(path).data.native_eval is False and load_config(None, []).data.native_eval is False
    assert load_config(path, ["data.native_eval=true"]).data.native_eval is True
    for bad in ("1", "yes_please", "[true]"):
        with pytest.raises(ValueError, match="native_eval"):
            load_config(path, [f"data.native_eval={bad}"])


def _ellipse(h, w, cy, cx, ry, rx, rot):
    y, x = np.mgrid[0:h, 0:w]
    y = (y + 0.5) / h - cy
    x = (x + 0.5) / w - cx
    c, s = np.cos(rot), np.sin(rot)
    u, v = c * x + s * y, -s * x + c * y
    return ((u / rx) ** 2 + (v / ry) ** 2 <= 1).astype(np.uint8)


def test_round_trip_beats_nearest_neighbour():
    """An ellipse at CAMUS-like sizes through the converter's nearest down-sampling to 256 x 256 and back: the rule's Dice against the native
    original is at least nearest neighbour's, in all twelve cases (DESIGN.md records the values)."""
    from convert_camus import resize
    dice = lambda a, b: 2 * int((a & b).sum()) / (int(a.sum()) + int(b.sum()))
    for (h0, w0) in [(549, 778), (1181, 972), (843, 512), (300, 400)]:
        for k in range(3):
            nat = _ellipse(h0, w0, 0.5 + 0.03 * k, 0.48, 0.31, 0.17 + 0.02 * k, 0.2 * k)
            small = resize(nat.astype(np.int64), 256, True).astype(np.uint8)
            lin = R.labels(small, h0, w0, 2)
            nn = R.nearest_labels(small, h0, w0)
            d_lin, d_nn = dice(lin, nat), dice(nn, nat)
            print(f"{h0} x {w0} ellipse {k}: nearest {d_nn:.5f} rule {d_lin:.5f} gain {d_lin - d_nn:+.5f}")
            assert d_lin >= d_nn, (h0, w0, k)
