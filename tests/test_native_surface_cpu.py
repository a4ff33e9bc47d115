"""CPU checks of the surface distances at native frame sizes: the reference (tests/native_surface_reference.py) against scipy's distance
transform with a sampling and against the reference of gdkvm_surface_distance_mm on uniform frames, ops.surface_distance_native's host
path against the reference on the ragged fixture, every refusal of the wrapper and of the C entry, the new config keys, the spacing of the
native pixel through the converter and the datasets."""
import filecmp
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

from tests import native_surface_reference as NR
from tests import spacing_reference as SR
from tests import surface_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SIZES = [(47, 61), (32, 32), (70, 45), (21, 90), (55, 54), (5, 7), (33, 31), (17, 65), (1, 1)]
SPACING = [(308, 154), (1, 4095), (4095, 1), (333, 471), (154, 308), (1000, 1000), (7, 3), (2048, 2047), (4095, 4095)]


def _clips(seed, T=2):
    rng = np.random.default_rng(seed)
    out = []
    for h0, w0 in SIZES:
        out.append(S.random_frames(T, h0, w0, seed=int(rng.integers(1 << 30))) if min(h0, w0) >= 17 else S.run_frames(T, h0, w0, seed=7)
                   if h0 * w0 > 1 else np.ones((T, 1, 1), np.uint8))
    return out


def test_reference_transform_against_scipy_with_a_sampling():
    """d2 = (ry dy)^2 + (rx dx)^2 is an integer: scipy's float distance, squared and rounded, must be that integer exactly (the products stay
    below 2^53 here), on frames of both orientations and with sides above 1024."""
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(0)
    for (h0, w0), (ry, rx) in (((47, 61), (308, 154)), ((21, 90), (1, 4095)), ((70, 45), (4095, 1)), ((1100, 3), (333, 471)), ((2, 1300), (7, 3))):
        surf = rng.random((h0, w0)) < 0.02
        surf[h0 // 2, w0 // 2] = True
        want = ndi.distance_transform_edt(~surf, sampling=(ry, rx))
        got = NR.edt2_um(surf, ry, rx)
        rebuilt = np.rint(want * want).astype(np.int64)
        assert np.array_equal(got, rebuilt), (h0, w0)


def test_reference_against_the_mm_reference_on_uniform_frames():
    for (h, w), sp in (((24, 20), (308, 154)), ((31, 47), (1, 4095)), ((1, 9), (471, 333))):
        a, b = S.case_frames(2, h, w, 1) if min(h, w) > 1 else (S.run_frames(3, h, w, 1), S.run_frames(3, h, w, 2))
        want = SR.surface_distance_mm_frames(a, b, sp, 1)
        got = NR.records([a], [b], [sp], 1)[0]
        assert np.array_equal(got, want), (h, w)


def test_closed_forms_at_the_bounds():
    """The extreme values the definition's bounds are stated for, in the reference and in ops' host path"""
    from gdkvm_amd import ops
    d2 = (2047 * 4095) ** 2
    assert 2 * d2 < 1 << 47 and (2 * d2) << 16 < 1 << 63
    for h0, w0 in ((2048, 1), (1, 2048)):
        m, g = np.zeros((1, h0, w0), np.uint8), np.zeros((1, h0, w0), np.uint8)
        m[0, 0, 0] = 1
        g[0, -1, -1] = 1
        want = [1, 1, d2, d2, math.isqrt(d2 << 16), math.isqrt(d2 << 16), d2, d2]
        assert NR.records([m], [g], [(4095, 4095)])[0, 0].tolist() == want
        got = ops.surface_distance_native(torch.from_numpy(m.reshape(-1)), torch.from_numpy(g.reshape(-1)), [(h0, w0)], 1, [(4095, 4095)])
        assert got[0, 0].tolist() == want


def test_ops_host_path_equals_the_reference_on_the_ragged_fixture():
    from gdkvm_amd import ops
    masks, targets = _clips(1), _clips(2)
    fm, sizes = NR.pack(masks)
    ft, _ = NR.pack(targets)
    assert sizes == SIZES
    for cls in (1, 2):
        want = NR.records(masks, targets, SPACING, cls)
        got = ops.surface_distance_native(torch.from_numpy(fm), torch.from_numpy(ft), sizes, 2, SPACING, cls=cls)
        assert got.dtype == torch.int64 and tuple(got.shape) == (len(SIZES), 2, 8)
        assert np.array_equal(got.numpy(), want)
    assert (want[:5, :, :2] > 0).all()
    # sizes and spacings as host tensors; the metrics helpers take the records unchanged
    got2 = ops.surface_distance_native(torch.from_numpy(fm), torch.from_numpy(ft), torch.tensor(sizes), 2, torch.tensor(SPACING, dtype=torch.int32), cls=2)
    assert torch.equal(got, got2)
    metrics, valid = ops.surface_metrics_mm(got)
    for b in range(len(SIZES)):
        for t in range(2):
            hd, hd95, assd, ok = NR.metrics_mm(want[b, t])
            assert bool(valid[b, t]) == ok and metrics[b, t].tolist() == pytest.approx([hd, hd95, assd], rel=1e-12, abs=0)


def test_ops_refusals_without_a_device():
    from gdkvm_amd import ops
    m = torch.zeros(2 * (30 + 21), dtype=torch.uint8)
    sizes, sp = [(5, 6), (7, 3)], [(300, 200), (100, 100)]
    f = ops.surface_distance_native
    assert tuple(f(m, m, sizes, 2, sp).shape) == (2, 2, 8)
    for bad in ([(0, 6), (7, 3)], [(5, 6), (7, 2049)]):
        with pytest.raises(ops.GdkvmError, match="outside 1..2048"):
            f(m, m, bad, 2, sp)
    for bad in ([(0, 200), (100, 100)], [(300, 200), (100, 4096)]):
        with pytest.raises(ops.GdkvmError, match="outside 1..4095"):
            f(m, m, sizes, 2, bad)
    with pytest.raises(ops.GdkvmError, match="sizes must be host integers"):
        f(m, m, torch.tensor(sizes, device="meta"), 2, sp)
    with pytest.raises(ops.GdkvmError, match="spacing_um must be host integers"):
        f(m, m, sizes, 2, torch.tensor(sp, device="meta"))
    with pytest.raises(ops.GdkvmError, match="1 spacings for 2 clips"):
        f(m, m, sizes, 2, sp[:1])
    with pytest.raises(ops.GdkvmError, match="no pair of integers"):
        f(m, m, sizes, 2, [(300.0, 200), (100, 100)])
    with pytest.raises(ops.GdkvmError, match="target must be a flat uint8 tensor of at least 102 bytes"):
        f(m, m[:-1], sizes, 2, sp)
    with pytest.raises(ops.GdkvmError, match="mask must be a flat uint8"):
        f(m.to(torch.int32), m, sizes, 2, sp)
    with pytest.raises(ops.GdkvmError, match="target must be a flat uint8"):
        f(m, m.reshape(2, -1), sizes, 2, sp)
    for cls in (255, -1, True):
        with pytest.raises(ops.GdkvmError, match="cls"):
            f(m, m, sizes, 2, sp, cls=cls)
    with pytest.raises(ops.GdkvmError, match="T = 0"):
        f(m, m, sizes, 0, sp)
    assert (ops.SURFACE_NATIVE_BAND_ROWS, ops.SURFACE_NATIVE_STRIP, ops.SURFACE_NATIVE_MAX_WG, ops.SURFACE_NATIVE_CLIPS) == (32, 64, 4096, 64)
    hdr = open(os.path.join(ROOT, "include", "gdkvm.h")).read()
    for name in ("BAND_ROWS", "STRIP", "MAX_WG", "CLIPS"):    # the header's macros are the module's constants
        assert f"#define GDKVM_SURFACE_NATIVE_{name} {getattr(ops, 'SURFACE_NATIVE_' + name)}\n" in hdr


def test_entry_refuses_bad_arguments_without_a_device():
    """The C entry validates everything before its first device call, so it answers on a machine without a GPU too."""
    from gdkvm_amd import ops
    lib = ops.load()
    sizes, sp = np.array([[5, 6], [7, 3]], np.int32), np.array([[300, 200], [100, 100]], np.int32)
    total, rows = 2 * (30 + 21), 2 * (5 + 7)
    m, t = np.zeros(total, np.uint8), np.zeros(total, np.uint8)
    need = lib.gdkvm_surface_distance_native_workspace_bytes(2, 2, total, rows)
    assert need > 0 and need % 16 == 0
    # an upper bound of the four integers only: 512 bytes of counts per frame, two bitmaps, two 16-bit planes, two list entries per pixel
    assert need >= 4 * 512 + 2 * 4 * (rows * 1) + 4 * total + 8 * total
    assert lib.gdkvm_surface_distance_native_workspace_bytes(2, 2, total + 64, rows + 4) >= need
    for bad in ((0, 2, total, rows), (2, 0, total, rows), (2, 2, 0, rows), (2, 2, total, 0), (-1, 2, total, rows), (1 << 20, 1 << 11, total, rows)):
        assert lib.gdkvm_surface_distance_native_workspace_bytes(*bad) == 0, bad
    wb = np.zeros(need + 32, np.uint8)
    w_al = wb.ctypes.data + (-wb.ctypes.data) % 16
    sb = np.zeros(4 * 8 + 4, np.int64)
    s_al = sb.ctypes.data + (-sb.ctypes.data) % 16

    def call(mask=m.ctypes.data, target=t.ctypes.data, sz=sizes, spc=sp, surf=s_al, nb=total, ws=w_al, wsb=need, clips=2, T=2, cls=1):
        return lib.gdkvm_surface_distance_native(mask, target, sz.ctypes.data if sz is not None else None,
                                                 spc.ctypes.data if spc is not None else None, surf, nb, ws, wsb, clips, T, cls, None)

    cases = [dict(clips=-1), dict(T=0), dict(cls=255), dict(cls=-1), dict(sz=np.array([[5, 6], [0, 3]], np.int32)),
             dict(sz=np.array([[2049, 6], [7, 3]], np.int32)), dict(spc=np.array([[0, 200], [100, 100]], np.int32)),
             dict(spc=np.array([[300, 200], [100, 4096]], np.int32)), dict(mask=None), dict(target=None), dict(sz=None), dict(spc=None),
             dict(surf=None), dict(surf=s_al + 8), dict(nb=total - 1), dict(ws=None), dict(wsb=need - 1), dict(ws=w_al + 4),
             dict(clips=1 << 16, T=1 << 15)]
    for kw in cases:
        assert call(**kw) == -1, kw
        assert b"surface_distance_native" in lib.gdkvm_last_error(), kw
    assert call(clips=0) == 0 and call(clips=0, mask=None, ws=None, wsb=0) == 0


def test_native_surface_config_keys():
    from gdkvm_amd.config import load_config
    path = os.path.join(ROOT, "config", "config_gdkvm_01.yaml")
    for cfg in (load_config(path), load_config(None, [])):
        assert cfg.data.native_surface_class == -1 and cfg.data.native_spacing_um is None
    cfg = load_config(path, ["data.native_eval=true", "data.native_surface_class=1", "data.native_spacing_um=[308,154]"])
    assert cfg.data.native_surface_class == 1 and cfg.data.native_spacing_um == [308, 154]
    with pytest.raises(ValueError, match="data.native_surface_class = 1 needs data.native_eval: true"):
        load_config(path, ["data.native_surface_class=1"])
    ncls = load_config(path).data.num_classes
    for bad in (str(ncls), "-2", "true", "1.5"):
        with pytest.raises(ValueError, match="native_surface_class"):
            load_config(path, ["data.native_eval=true", f"data.native_surface_class={bad}"])
    for bad in ("[308]", "[0,154]", "[308,4096]", "308", "[308.0,154]"):
        with pytest.raises(ValueError, match="native_spacing_um"):
            load_config(path, [f"data.native_spacing_um={bad}"])


def _tiny_camus(src, rng):
    from convert_camus import write_nifti
    for pid, (w, h, f), pix in (("patient0001", (13, 17, 6), (0.308, 0.154)), ("patient0002", (20, 11, 3), (0.3, 5.0))):
        os.makedirs(os.path.join(src, pid))
        for view in ("2CH", "4CH"):
            write_nifti(os.path.join(src, pid, f"{pid}_{view}_half_sequence.nii.gz"), rng.integers(0, 255, (w, h, f)).astype(np.uint8), pix)
            write_nifti(os.path.join(src, pid, f"{pid}_{view}_half_sequence_gt.nii.gz"), rng.integers(0, 4, (w, h, f)).astype(np.uint8), pix)


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_converter_native_spacing_and_the_tables(tmp_path):
    from convert_camus import convert
    from gdkvm_amd.config import load_config
    from gdkvm_amd.data import CamusPng, NpzClips, SyntheticEchoClips, native_spacing_table
    src, plain, nat = str(tmp_path / "src"), str(tmp_path / "plain"), str(tmp_path / "nat")
    _tiny_camus(src, np.random.default_rng(3))
    lines = []
    convert(src, plain, size=8, frames=4, split="val", log=lambda *a: None)
    convert(src, nat, size=8, frames=4, split="val", log=lines.append, native_spacing=True)
    # without the flag the tree is what it was, file for file; the flag only adds native_spacing.json, and spacing.json keeps its content
    assert not any("native_spacing" in f for f in _tree(plain))
    extra = [f for f in _tree(nat) if "native_spacing" in f]
    assert sorted(set(_tree(nat)) - set(extra)) == _tree(plain)
    assert all(filecmp.cmp(os.path.join(plain, f), os.path.join(nat, f), shallow=False) for f in _tree(plain))
    # patient0001: pixdim (x, y) = (0.308, 0.154) mm -> [row_um, col_um] = [154, 308]; patient0002: 5 mm is outside 1..4095 um: no file, a line
    assert extra == [os.path.join("val", "patient0001", v, "native_spacing.json") for v in ("2CH", "4CH")]
    with open(os.path.join(nat, extra[0])) as f:
        assert json.load(f) == {"spacing_um": [154, 308]}
    assert sum("no usable native pixel spacing" in ln for ln in lines) == 2 and all("patient0002" in ln for ln in lines if "native pixel" in ln)
    cfg = load_config(None, [])
    ds = CamusPng(nat, "val", 4, as_uint8=True)
    assert [ds.native_spacing_um(i) for i in range(4)] == [(154, 308), (154, 308), None, None]
    assert native_spacing_table(ds, cfg) is None              # a table with holes is no table
    cfg_fb = load_config(None, ["data.native_spacing_um=[200,100]"])
    tab = native_spacing_table(ds, cfg_fb)
    assert tab.dtype == torch.int32 and tab.device.type == "cpu" and tab.tolist() == [[154, 308], [154, 308], [200, 100], [200, 100]]
    assert native_spacing_table(CamusPng(plain, "val", 4, as_uint8=True), cfg) is None
    with open(os.path.join(nat, extra[1]), "w") as f:
        f.write("{not json")
    assert ds.native_spacing_um(1) is None
    # NpzClips: an optional native_spacing_um array, as spacing_um is
    root = tmp_path / "npz" / "val"
    os.makedirs(root)
    fr = np.zeros((3, 8, 8), np.uint8)
    np.savez(root / "a.npz", frames=fr, masks=fr, native_spacing_um=np.asarray([308, 154], np.int32))
    np.savez(root / "b.npz", frames=fr, masks=fr, native_spacing_um=np.asarray([1, 4095], np.int64))
    dn = NpzClips(str(tmp_path / "npz"), "val", 3, as_uint8=True)
    assert dn.native_spacing_um(0) == (308, 154) and native_spacing_table(dn, cfg).tolist() == [[308, 154], [1, 4095]]
    np.savez(root / "c.npz", frames=fr, masks=fr, native_spacing_um=np.asarray([308, 4096], np.int32))
    np.savez(root / "d.npz", frames=fr, masks=fr, spacing_um=np.asarray([308, 154], np.int32))
    dn = NpzClips(str(tmp_path / "npz"), "val", 3, as_uint8=True)
    assert dn.native_spacing_um(2) is None and dn.native_spacing_um(3) is None and native_spacing_table(dn, cfg) is None
    assert native_spacing_table(dn, cfg_fb).tolist() == [[308, 154], [1, 4095], [200, 100], [200, 100]]
    # the other datasets have none; a dataset without the method falls back to the configured pair
    syn = SyntheticEchoClips(2, 3, 16)
    assert syn.native_spacing_um(0) is None and native_spacing_table(syn, cfg) is None
    assert native_spacing_table([0, 1], cfg_fb).tolist() == [[200, 100], [200, 100]]
