"""Native-resolution input without a device: tests/native_input_reference.py (the rule of gdkvm_frames_from_native in include/gdkvm.h) against
its own fixed points and against torch's avg_pool2d at integer ratios, ops.frames_from_native's host path and refusals, the C entry's
refusals, the converter's --native-frames / --resample area, the datasets' native frames and predict.py's input readers.  segment_native's
forward has no CPU path (model.segment runs HIP kernels only), so its composition is tested on the GPU (tests/test_native_input_gpu.py)
and here only its refusal of a CPU model."""
import filecmp
import io
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests import native_input_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_weight_facts():
    """The three facts the header states about wy, on the shapes the issue lists"""
    for h0, H in ((7, 4), (5, 3), (3, 8), (549, 16), (778, 16), (1, 4), (2048, 5), (3, 2), (64, 64)):
        w = R.weights(H, h0)
        assert (w.sum(1) == h0).all() and (w.sum(0) == H).all()
        for i in range(H):
            nz = np.nonzero(w[i])[0]
            assert nz[0] == (i * h0) // H and nz[-1] == -((-(i + 1) * h0) // H) - 1 and len(nz) == nz[-1] - nz[0] + 1


def test_restatement_fixed_points():
    rng = np.random.default_rng(0)
    v = rng.integers(0, 256, (3, 9, 13), dtype=np.uint8)
    assert np.array_equal(R.area_bytes(v, 9, 13), v)                                       # identity
    full = np.full((2048, 2048), 255, np.uint8)                                            # the 32-bit bound: 2 N + h0 w0 = 511 * 2^22 < 2^32
    assert R.numerators(full, 1, 1).item() == 255 * 2 ** 22 and 2 * R.numerators(full, 1, 1).item() + 2 ** 22 < 2 ** 32
    assert R.area_bytes(full, 1, 1).tolist() == [[255]]
    for (h0, w0), (H, W) in (((7, 5), (4, 3)), ((3, 3), (8, 8)), ((549, 778), (16, 16)), ((1, 1), (4, 4)), ((2048, 3), (5, 2))):
        v = rng.integers(0, 256, (h0, w0), dtype=np.uint8)
        assert R.numerators(v, H, W).sum() == H * W * int(v.astype(np.int64).sum())       # mass
        c = np.full((h0, w0), 77, np.uint8)
        assert (R.area_bytes(c, H, W) == 77).all()                                         # a constant frame stays constant
    one = lambda rows: R.area_bytes(np.array(rows, np.uint8), 1, 1).item()
    assert one([[0, 0], [0, 1]]) == 0 and one([[1, 1], [0, 0]]) == 1 and one([[0, 1], [1, 1]]) == 1     # round half up
    v = np.tile(np.array([0, 0, 255], np.uint8), (3, 1))
    assert (R.area_bytes(v, 8, 8) == np.array([0, 0, 0, 0, 0, 170, 255, 255], np.uint8)).all()


def test_restatement_against_avg_pool_at_integer_ratios():
    rng = np.random.default_rng(1)
    for (h0, w0), (H, W) in (((12, 20), (4, 5)), ((16, 16), (8, 8)), ((9, 6), (3, 6)), ((30, 7), (5, 1))):
        v = rng.integers(0, 256, (4, h0, w0), dtype=np.uint8)
        want = torch.floor(TF.avg_pool2d(torch.from_numpy(v).double()[:, None], (h0 // H, w0 // W))[:, 0] + 0.5).to(torch.uint8)
        assert np.array_equal(R.area_bytes(v, H, W), want.numpy())


def test_output_dtypes_are_the_prefetcher_s_cast():
    q = torch.arange(256, dtype=torch.uint8)
    f32 = torch.mul(q, 1.0 / 255.0, out=torch.empty(256, dtype=torch.float32))
    bf = torch.mul(q, 1.0 / 255.0, out=torch.empty(256, dtype=torch.bfloat16))
    assert np.array_equal(R.to_float32(q.numpy()).view(np.uint32), f32.numpy().view(np.uint32))
    assert np.array_equal(R.to_bf16_bits(q.numpy()), bf.view(torch.int16).numpy().view(np.uint16))


def _ragged(rng, T=3):
    clips = [rng.integers(0, 256, (T, h0, w0), dtype=np.uint8) for h0, w0 in ((7, 5), (5, 7), (1, 1), (3, 3), (33, 17), (8, 8))]
    return R.pack(clips)


def test_ops_host_path_equals_the_restatement():
    from gdkvm_amd import ops
    flat, sizes = _ragged(np.random.default_rng(2))
    ft = torch.from_numpy(flat)
    for H, W in ((4, 3), (8, 8)):
        for C in (1, 3):
            ref, offs = R.frames_from_native(flat, sizes, 3, H, W, C)
            out, o2 = ops.frames_from_native(ft, sizes, 3, grid=(H, W), channels=C, dtype=torch.uint8)
            assert o2 == offs and out.dtype == torch.uint8 and np.array_equal(out.numpy(), ref)
            out, _ = ops.frames_from_native(ft, torch.tensor(sizes, dtype=torch.int32), 3, grid=(H, W), channels=C, dtype=torch.float32)
            assert np.array_equal(out.numpy().view(np.uint32), R.to_float32(ref).view(np.uint32))
            buf = torch.empty((len(sizes), 3, C, H, W), dtype=torch.bfloat16)
            out, _ = ops.frames_from_native(ft, sizes, 3, grid=(H, W), channels=C, dtype=torch.bfloat16, out=buf)
            assert out is buf and np.array_equal(out.view(torch.int16).numpy().view(np.uint16), R.to_bf16_bits(ref))
    one = ops.native_frames(ft, sizes, 3, 4)
    got, _ = ops.frames_from_native(one.reshape(-1), [sizes[4]], 3, grid=(8, 8), channels=1, dtype=torch.uint8)
    assert np.array_equal(got.numpy(), R.frames_from_native(flat, sizes, 3, 8, 8, 1)[0][4:5])
    assert "gdkvm_frames_from_native" in ops.SIGNATURES and "gdkvm_frames_from_native_workspace_bytes" in ops.SIGNATURES


def test_ops_refusals_without_a_device():
    from gdkvm_amd import ops
    sizes = [(5, 6), (7, 3)]
    total = 2 * (30 + 21)
    flat = torch.zeros(total, dtype=torch.uint8)
    bad = [(dict(flat=flat.to(torch.int32)), "flat must be a flat uint8"), (dict(flat=flat.reshape(2, -1)), "flat must be a flat uint8"),
           (dict(flat=flat[:-1]), f"take {total} bytes, flat holds {total - 1}"), (dict(T=0), "T = 0"), (dict(T=True), "T = True"),
           (dict(grid=(4, 1025)), r"each in 1\.\.1024"), (dict(grid=(0, 4)), r"each in 1\.\.1024"), (dict(grid=4), "must be a pair"),
           (dict(grid=(4.0, 4)), "must be integers"), (dict(channels=0), "channels = 0"), (dict(channels=5), "channels = 5"),
           (dict(dtype=torch.float16), "none of uint8, float32, bfloat16"), (dict(sizes=[(5, 6), (0, 3)]), r"sizes\[1\] = 0 x 3 outside 1..2048"),
           (dict(sizes=[(5, 6), (7, 2049)]), "outside 1..2048"), (dict(sizes=[(5, 6), (7.0, 3)]), "no pair of integers"),
           (dict(sizes=5), "sizes must be a sequence"), (dict(sizes=torch.ones((2, 2), dtype=torch.int32, device="meta")), "sizes must be host integers"),
           (dict(out=torch.zeros((2, 2, 3, 4, 4))), "out must be torch.uint8"), (dict(out=torch.zeros((2, 2, 3, 4, 5), dtype=torch.uint8)), "out must be")]
    for kw, msg in bad:
        args = {"flat": flat, "sizes": sizes, "T": 2, "grid": (4, 4), "channels": 3, "dtype": torch.uint8, **kw}
        with pytest.raises(ops.GdkvmError, match="frames_from_native: .*" + msg):
            ops.frames_from_native(**args)


def test_entry_refuses_bad_arguments_without_a_device():
    """The C entry validates everything before its first device call, so it answers on a machine without a GPU too."""
    from gdkvm_amd import ops
    lib = ops.load()
    sizes = np.array([[5, 6], [7, 3]], np.int32)
    total = 2 * (30 + 21)
    nat = np.zeros(total + 64, np.uint8)
    ob = np.zeros(2 * 2 * 3 * 4 * 4 * 4 + 32, np.uint8)
    o_al = ob.ctypes.data + (-ob.ctypes.data) % 16

    def call(native=nat.ctypes.data, sz=sizes, o=o_al, nb=total, clips=2, T=2, C=3, H=4, W=4, dt=1):
        return lib.gdkvm_frames_from_native(native, sz.ctypes.data if sz is not None else None, o, nb, None, 0, clips, T, C, H, W, dt, None)

    cases = [dict(clips=-1), dict(T=0), dict(H=0), dict(W=1025), dict(C=0), dict(C=5), dict(dt=3), dict(dt=-1),
             dict(sz=np.array([[5, 6], [0, 3]], np.int32)), dict(sz=np.array([[5, 6], [7, 2049]], np.int32)), dict(native=None), dict(sz=None),
             dict(o=None), dict(o=o_al + 4), dict(nb=total - 1), dict(o=nat.ctypes.data + (-nat.ctypes.data) % 16)]
    for kw in cases:
        assert call(**kw) == -1, kw
        assert b"frames_from_native" in lib.gdkvm_last_error(), kw
    assert call(clips=0) == 0
    assert lib.gdkvm_frames_from_native_workspace_bytes(16, 10, 3, 256, 256, 2) == 0


def _tiny_camus(src, rng):
    from convert_camus import write_nifti
    for pid, (w, h, f), dt, top in (("patient0001", (13, 17, 6), np.uint8, 255), ("patient0002", (20, 11, 3), np.int16, 900)):
        os.makedirs(os.path.join(src, pid))
        for view in ("2CH", "4CH"):
            write_nifti(os.path.join(src, pid, f"{pid}_{view}_half_sequence.nii.gz"), rng.integers(0, top, (w, h, f)).astype(dt), (0.3, 0.2))
            write_nifti(os.path.join(src, pid, f"{pid}_{view}_half_sequence_gt.nii.gz"), rng.integers(0, 4, (w, h, f)).astype(np.uint8), (0.3, 0.2))


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_converter_native_frames_area_resample_and_datasets(tmp_path):
    from PIL import Image
    from convert_camus import convert, read_nifti, resize
    from gdkvm_amd import ops
    from gdkvm_amd.data import CamusPng, NpzClips
    from gdkvm_amd.predict import load_input
    src, plain, area = str(tmp_path / "src"), str(tmp_path / "plain"), str(tmp_path / "area")
    _tiny_camus(src, np.random.default_rng(3))
    quiet = lambda *a: None
    convert(src, plain, size=8, frames=4, split="val", log=quiet)
    convert(src, area, size=8, frames=4, split="val", log=quiet, native_frames=True, resample="area")
    # without the flags: the file set and the bytes of the code path of before (restated here: bilinear resize, 255 / max when above 255)
    assert not any("native_" in f for f in _tree(plain)) and len(_tree(plain)) == 4 * (4 + 3) + 4
    for pid, view, n_fr, picks in (("patient0001", "2CH", 6, 4), ("patient0002", "4CH", 3, 3)):
        img = read_nifti(os.path.join(src, pid, f"{pid}_{view}_half_sequence.nii.gz"))
        pick = np.round(np.linspace(0, n_fr - 1, 4)).astype(int) if n_fr >= 4 else np.arange(n_fr)
        assert len(pick) == picks
        for j, f in enumerate(pick):
            a = resize(np.asarray(img[:, :, f]).T, 8, False)
            hi = float(a.max()) or 1.0
            buf = io.BytesIO()
            Image.fromarray(np.clip(a * (255.0 / hi if hi > 255.0 else 1.0), 0, 255).astype(np.uint8)).save(buf, format="PNG")
            with open(os.path.join(plain, "val", pid, view, f"frame_{j:03d}.png"), "rb") as fh:
                assert fh.read() == buf.getvalue(), (pid, view, j)
    # with them: the flags only add native_frame files; masks and spacing are untouched; frame == rule(native_frame) byte for byte
    extra = [f for f in _tree(area) if "native_frame" in f]
    assert sorted(set(_tree(area)) - set(extra)) == _tree(plain) and len(extra) == 2 * (4 + 3)
    assert all(filecmp.cmp(os.path.join(plain, f), os.path.join(area, f), shallow=False) for f in _tree(plain) if "frame_" not in f)
    for f in extra:
        nat = np.asarray(Image.open(os.path.join(area, f)))
        fr = np.asarray(Image.open(os.path.join(area, f.replace("native_frame_", "frame_"))))
        assert nat.dtype == np.uint8 and fr.dtype == np.uint8 and np.array_equal(fr, R.area_bytes(nat, 8, 8)), f
        got, _ = ops.frames_from_native(torch.from_numpy(nat.copy()).reshape(-1), [nat.shape], 1, grid=(8, 8), channels=1, dtype=torch.uint8)
        assert np.array_equal(got[0, 0, 0].numpy(), fr)
    # the native frame is the stored frame, scaled by 255 / max when the maximum exceeds 255
    img = read_nifti(os.path.join(src, "patient0002", "patient0002_2CH_half_sequence.nii.gz"))
    a = np.asarray(img[:, :, 1]).T.astype(np.float32)
    want = np.clip(a * (255.0 / float(a.max())), 0, 255).astype(np.uint8)
    assert a.max() > 255 and np.array_equal(np.asarray(Image.open(os.path.join(area, "val", "patient0002", "2CH", "native_frame_001.png"))), want)
    # CamusPng.native_frames: the PNGs at the frame pick of __getitem__; None for a tree without them or with a picked one missing
    ds = CamusPng(area, "val", 4, as_uint8=True)
    n0 = ds.native_frames(0)
    assert n0.dtype == torch.uint8 and tuple(n0.shape) == (4, 17, 13)
    for j in range(4):
        assert np.array_equal(n0[j].numpy(), np.asarray(Image.open(os.path.join(area, "val", "patient0001", "2CH", f"native_frame_{j:03d}.png"))))
    n2 = ds.native_frames(2)                                  # 3 frames on disk, T = 4: the last repeats, as in __getitem__
    assert tuple(n2.shape) == (4, 11, 20) and torch.equal(n2[3], n2[2])
    assert torch.equal(CamusPng(area, "val", 2, as_uint8=True).native_frames(0), n0[[0, 3]])
    # ... and what the dataset hands the model is the rule applied to them, in every plane
    x, _ = ds[0]
    assert np.array_equal(x.numpy(), R.frames_from_native(n0.numpy().reshape(-1), [(17, 13)], 4, 8, 8, 3)[0][0])
    assert CamusPng(plain, "val", 4, as_uint8=True).native_frames(0) is None
    # predict.py's directory reader: the native frames, and spacing.json rescaled back to the native pixel
    name, fr, sp = load_input(os.path.join(area, "val", "patient0001", "2CH"))
    with open(os.path.join(area, "val", "patient0001", "2CH", "spacing.json")) as fh:
        meta = json.load(fh)
    assert name == "2CH" and tuple(fr.shape) == (4, 17, 13) and torch.equal(fr, n0) and meta["native_hw"] == [17, 13]
    assert sp == (meta["spacing_um"][0] * 8 / 17, meta["spacing_um"][1] * 8 / 13)
    _, fr_plain, sp_plain = load_input(os.path.join(plain, "val", "patient0001", "2CH"))
    assert tuple(fr_plain.shape) == (4, 8, 8) and sp_plain == (float(meta["spacing_um"][0]), float(meta["spacing_um"][1]))
    os.remove(os.path.join(area, "val", "patient0001", "2CH", "native_frame_003.png"))
    assert ds.native_frames(0) is None
    # NpzClips: an optional native_frames array
    root = tmp_path / "npz" / "val"
    os.makedirs(root)
    z8 = np.zeros((3, 8, 8), np.uint8)
    nf = np.random.default_rng(4).integers(0, 256, (4, 5, 9)).astype(np.uint8)
    np.savez(root / "a.npz", frames=z8, masks=z8, native_frames=nf)
    np.savez(root / "b.npz", frames=z8, masks=z8)
    np.savez(root / "c.npz", frames=z8, masks=z8, native_frames=nf[:2])
    dn = NpzClips(str(tmp_path / "npz"), "val", 3, as_uint8=True)
    assert np.array_equal(dn.native_frames(0).numpy(), nf[:3]) and dn.native_frames(1) is None and dn.native_frames(2) is None


def test_predict_inputs_and_grid_spacing(tmp_path):
    from gdkvm_amd import ops
    from gdkvm_amd.config import load_config
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    from gdkvm_amd.predict import grid_spacing_um, load_input, segment_native
    clip = np.random.default_rng(5).integers(0, 256, (3, 9, 7), dtype=np.uint8)
    np.save(tmp_path / "a.npy", clip)
    np.savez(tmp_path / "b.npz", frames=clip, spacing_um=np.array([150.5, 220.0]))
    name, fr, sp = load_input(str(tmp_path / "a.npy"))
    assert name == "a" and sp is None and np.array_equal(fr.numpy(), clip)
    name, fr, sp = load_input(str(tmp_path / "b.npz"))
    assert name == "b" and sp == (150.5, 220.0) and np.array_equal(fr.numpy(), clip)
    np.save(tmp_path / "c.npy", clip.astype(np.float32))
    with pytest.raises(ValueError, match=r"uint8 \[T, h0, w0\]"):
        load_input(str(tmp_path / "c.npy"))
    with pytest.raises(ValueError, match="neither a .npy"):
        load_input(str(tmp_path / "nothing.txt"))
    # the converter's formula: rint(um * native / grid); outside 1..4095 there is no mL
    assert grid_spacing_um((154.0, 154.0), 549, 778, 256, 256) == (int(np.rint(154.0 * 549 / 256)), int(np.rint(154.0 * 778 / 256)))
    assert grid_spacing_um((154.0, 154.0), 2048, 2048, 8, 8) is None and grid_spacing_um((0.1, 154.0), 8, 8, 8, 8) is None
    assert grid_spacing_um((float("nan"), 1.0), 8, 8, 8, 8) is None and grid_spacing_um(None, 8, 8, 8, 8) is None
    # no CPU path for the forward: a CPU model is refused, loudly
    torch.manual_seed(0)
    model = GDKVM(GDKVMConfig(widths=(16, 32, 64), pixel_dim=64, value_dim=32)).eval()
    cfg = load_config(None, ["data.size=32", "precision=fp32"])
    with pytest.raises(ops.GdkvmError, match="segment_native: the model must be on a HIP device"):
        segment_native(model, cfg, [torch.from_numpy(clip)])
