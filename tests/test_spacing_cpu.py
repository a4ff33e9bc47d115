"""The measurements with a pixel spacing, without a device: tests/spacing_reference.py (the definition of gdkvm_surface_distance_mm and
gdkvm_lv_measure_mm in include/gdkvm.h) against scipy, against the pixel references it extends, and against closed forms; and the spacing's way
from a NIfTI header through tools/convert_camus.py, gdkvm_amd.data and the configuration."""
import json
import math
import os

import numpy as np
import pytest

from tests import lv_reference as R
from tests import spacing_reference as P
from tests import surface_reference as S

Q = P.Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPACINGS = [(330, 468), (1, 4095), (4095, 1), (4095, 4095), (3, 7)]


def test_edt2_um_equals_scipys_sampled_transform():
    """scipy's exact Euclidean transform with sampling = (ry, rx) is a float distance; squared and rounded it is the integer (its error is
    far below one half: d < 2^23 um carries 2^-29 um of fp64 rounding, d d about 2^-5 um^2 at most)."""
    ndi = pytest.importorskip("scipy.ndimage")
    for frames in (S.random_frames(2, 30, 58, seed=3), S.random_frames(2, 41, 35, seed=4)):
        for f in range(frames.shape[0]):
            for cls in (1, 2):
                sf = S.surface(frames[f] == cls)
                assert sf.any()
                for ry, rx in SPACINGS:
                    want = np.rint(ndi.distance_transform_edt(~sf, sampling=(ry, rx)) ** 2).astype(np.int64)
                    assert np.array_equal(P.edt2_um(sf, ry, rx), want), (f, cls, ry, rx)


def test_unit_spacing_is_the_pixel_reference_and_a_common_factor_scales():
    mask, target = S.case_frames(2, 30, 58, 1)
    for f in range(mask.shape[0]):
        pix = S.surface_distance_ref(mask[f], target[f], 1)
        one = P.surface_distance_mm_ref(mask[f], target[f], 1, 1, 1)
        assert [one[i] for i in (0, 1, 2, 3, 6, 7)] == [pix[i] for i in (0, 1, 2, 3, 6, 7)], f
        for s in (7, 4095):
            rec = P.surface_distance_mm_ref(mask[f], target[f], s, s, 1)
            assert rec[:2] == pix[:2] and [rec[i] for i in (2, 3, 6, 7)] == [pix[i] * s * s for i in (2, 3, 6, 7)], (f, s)
    sf = S.surface(mask[0] == 1)
    assert np.array_equal(P.edt2_um(sf, 1, 1), S.edt2(sf)) and np.array_equal(P.edt2_um(sf, 13, 13), 169 * S.edt2(sf))


def test_transposed_frames_with_swapped_spacing_give_the_same_record():
    mask, target = S.case_frames(2, 30, 58, 2)
    for f in range(mask.shape[0]):
        for ry, rx in ((330, 468), (1, 4095)):
            a = P.surface_distance_mm_ref(mask[f], target[f], ry, rx, 2)
            b = P.surface_distance_mm_ref(np.ascontiguousarray(mask[f].T), np.ascontiguousarray(target[f].T), rx, ry, 2)
            assert a == b, (f, ry, rx)


def test_records_of_the_corner_cases():
    z = np.zeros((5, 9), np.uint8)
    m = z.copy(); m[2, 1] = 1
    t = z.copy(); t[4, 7] = 1
    d2 = (2 * 330) ** 2 + (6 * 468) ** 2
    r = math.isqrt(d2 << 16)
    assert P.surface_distance_mm_ref(m, t, 330, 468) == [1, 1, d2, d2, r, r, d2, d2]
    assert P.surface_distance_mm_ref(m, z, 330, 468) == [1, 0, 0, 0, 0, 0, 0, 0]
    assert P.surface_distance_mm_ref(m, t, 0, 468) == [-1] * 8 and P.surface_distance_mm_ref(m, t, 330, 4096) == [-1] * 8
    hd, hd95, assd, ok = P.metrics_mm_ref([1, 1, d2, d2, r, r, d2, d2])
    assert ok and hd == hd95 == math.sqrt(d2) / 1000 and 0 <= math.sqrt(d2) / 1000 - assd < 2.0 ** -8 / 1000 + 1e-15
    assert P.metrics_mm_ref([-1] * 8) == (0.0, 0.0, 0.0, False) and P.metrics_mm_ref([3, 0, 0, 0, 0, 0, 0, 0])[3] is False
    # a column without a surface pixel offers nothing, however small ry makes the square of "none"
    m = z.copy(); m[0, 0] = 1
    t = z.copy(); t[0, 8] = 1
    assert P.surface_distance_mm_ref(m, t, 1, 4095)[2] == (8 * 4095) ** 2


def _rect(H, W, y0, x0, h, w):
    m = np.zeros((H, W), np.uint8)
    m[y0:y0 + h, x0:x0 + w] = 1
    return m


@pytest.mark.parametrize("w,h,ry,rx", [(12, 40, 330, 468), (50, 12, 468, 330), (40, 12, 100, 4095), (30, 31, 300, 310), (16, 16, 500, 300)])
def test_axis_aligned_rectangles_have_the_cylinders_volume(w, h, ry, rx):
    """An axis-aligned rectangle of w x h pixels: every disk holds the same area, so V = pi (short side)^2 (long side) / 4 up to rounding."""
    res = P.lv_measure_mm_ref(_rect(64, 64, 7, 5, h, w), ry, rx, 1, 20)
    n, Vx, Vy, Lt, E = res["stats"][0], res["stats"][6], res["stats"][7], res["stats"][10], res["stats"][11]
    wm, hm = w * rx / 1000, h * ry / 1000
    long_, short = max(wm, hm), min(wm, hm)
    assert (Vx == 0) != (Vy == 0)                             # the axis lies along the rows or along the columns
    assert res["geom"][0] == pytest.approx(long_, rel=1e-14) and res["geom"][1] == pytest.approx(math.pi * short * short * long_ / 4 / 1000, rel=1e-13)
    assert res["geom"][5] == pytest.approx(wm * hm, rel=1e-15) and res["geom"][4] == pytest.approx(ry if Vx == 0 else rx, rel=1e-15)
    assert res["geom"][2] == pytest.approx((5 + (w - 1) / 2) * rx / 1000, rel=1e-15) and res["geom"][3] == pytest.approx((7 + (h - 1) / 2) * ry / 1000, rel=1e-15)
    assert sum(res["disks"]) == n * 20 * n * E and 16 <= E <= Q and Lt == n * E * (h if Vx == 0 else w)


def test_isotropic_spacing_reproduces_the_pixel_measurement():
    for deg in (0, 30, 45, 90):
        m = R.ellipse_mask(128, 128, 63.5, 63.5, 45, 18, deg)
        pix, mm = R.lv_measure_ref(m), P.lv_measure_mm_ref(m, 300, 300)
        assert mm["stats"][:11] == pix["stats"][:11] and mm["stats"][11] == Q and mm["disks"] == pix["disks"]
        assert mm["geom"][4] == 300.0 and mm["geom"][0] == pytest.approx(pix["geom"][0] * 0.3, rel=1e-15)
        # the same integers through D + 8 differently ordered fp64 roundings
        assert mm["geom"][1] == pytest.approx(pix["geom"][1] * 0.3 ** 3 / 1000, rel=1e-14)


def test_rasterised_ellipses_on_anisotropic_pixels_are_close_to_the_prolate_spheroid():
    """Semi-axes 35 x 15 mm on a 256 x 256 grid of 0.330 x 0.468 mm pixels: the volume is that of the spheroid whatever the ellipse's
    direction -- in pixel units the same ventricle would change its shape with the angle."""
    ry, rx, la, sa = 330, 468, 35.0, 15.0
    want = 4.0 / 3.0 * math.pi * la * sa * sa / 1000
    yy, xx = np.mgrid[0:256, 0:256].astype(np.float64)
    dy, dx = (yy - 127.5) * ry / 1000, (xx - 127.5) * rx / 1000
    for deg in (0, 30, 45, 90):
        th = math.radians(deg)
        al, ac = dx * math.sin(th) + dy * math.cos(th), dx * math.cos(th) - dy * math.sin(th)
        m = ((al / la) ** 2 + (ac / sa) ** 2 <= 1.0).astype(np.uint8)
        res = P.lv_measure_mm_ref(m, ry, rx)
        n, E = res["stats"][0], res["stats"][11]
        assert abs(res["geom"][1] - want) <= 0.0075 * want, (deg, res["geom"][1] / want)
        assert res["geom"][0] == pytest.approx(2 * la, rel=0.02) and sum(res["disks"]) == n * 20 * n * E
        ux, uy = res["stats"][6] / Q * max(ry, rx) / rx, res["stats"][7] / Q * max(ry, rx) / ry      # back to the physical unit vector
        assert abs(abs(ux) - abs(math.sin(th))) < 0.01 and abs(abs(uy) - abs(math.cos(th))) < 0.01, (deg, ux, uy)


@pytest.mark.parametrize("ry,rx", [(1, 4095), (4095, 1)])
def test_integer_ranges_hold_at_a_full_frame(ry, rx):
    """1024 x 1024 with every pixel of the class, and one full line along the FINE direction (the smallest E there is): |V| <= Q,
    16 <= E <= Q and D Lt < 2^62 (asserted inside the reference too) with 64 disks."""
    full = np.ones((1024, 1024), np.uint8)
    line = np.zeros((1024, 1024), np.uint8)
    if ry < rx:
        line[:, 500] = 1
    else:
        line[500, :] = 1
    for m, e_want in ((full, Q), (line, 16)):
        res = P.lv_measure_mm_ref(m, ry, rx, 1, 64)
        n, Vx, Vy, Lt, E = (res["stats"][i] for i in (0, 6, 7, 10, 11))
        assert abs(Vx) <= Q and abs(Vy) <= Q and 16 <= E <= Q and E == e_want and 64 * Lt < 1 << 62
        assert sum(res["disks"]) == n * 64 * n * E
        assert res["geom"][0] == pytest.approx(1024 * (max(ry, rx) if m is full else min(ry, rx)) / 1000, rel=1e-3)


def test_out_of_range_spacing_and_empty_frames():
    m = _rect(16, 16, 2, 2, 5, 3)
    assert P.lv_measure_mm_ref(m, 0, 300) == {"stats": [-1] * 12, "disks": [-1] * 20, "geom": [-1.0] * 6}
    assert P.lv_measure_mm_ref(m, 300, 4096, D=7)["disks"] == [-1] * 7
    assert P.lv_measure_mm_ref(m, 300, 300, cls=2) == {"stats": [0] * 12, "disks": [0] * 20, "geom": [0.0] * 6}


# ---- the spacing's way from the files to eval.py -------------------------------------------------------------------------------------------------
def _camus_tree(src, pixdim, unit=None):
    from tools.convert_camus import write_nifti
    rng = np.random.default_rng(2)
    (src / "patient0001").mkdir(parents=True)
    for view in ("2CH", "4CH"):
        img = rng.integers(0, 255, (60, 90, 3), dtype=np.uint8)              # stored [x, y, frame]: 60 wide, 90 high
        lab = np.zeros((60, 90, 3), np.uint8)
        lab[20:40, 20:70] = 1
        for name, arr in ((f"patient0001_{view}_half_sequence.nii.gz", img), (f"patient0001_{view}_half_sequence_gt.nii.gz", lab)):
            write_nifti(str(src / "patient0001" / name), arr, **({} if pixdim is None else {"pixdim": pixdim}))


def test_write_nifti_without_pixdim_writes_the_bytes_it_wrote_before(tmp_path):
    import gzip
    import struct
    from tools.convert_camus import read_nifti, read_nifti_pixdim_mm, write_nifti
    arr = np.arange(2 * 3 * 4, dtype=np.uint8).reshape(2, 3, 4)
    write_nifti(str(tmp_path / "a.nii"), arr)
    hdr = bytearray(352)                                         # the header as the writer has always laid it out
    struct.pack_into("<i", hdr, 0, 348)
    struct.pack_into("<8h", hdr, 40, 3, 2, 3, 4, 1, 1, 1, 1)
    struct.pack_into("<h", hdr, 70, 2)
    struct.pack_into("<h", hdr, 72, 8)
    struct.pack_into("<f", hdr, 108, 352.0)
    struct.pack_into("<2f", hdr, 112, 1.0, 0.0)
    hdr[344:348] = b"n+1\0"
    assert open(tmp_path / "a.nii", "rb").read() == bytes(hdr) + np.asfortranarray(arr).tobytes(order="F")
    write_nifti(str(tmp_path / "b.nii.gz"), arr, pixdim=(0.2, 0.3))
    raw = gzip.open(tmp_path / "b.nii.gz", "rb").read()
    assert struct.unpack("<2f", raw[80:88]) == (np.float32(0.2), np.float32(0.3)) and raw[123] == 2
    diff = [i for i in range(352) if raw[i] != hdr[i]]
    assert set(diff) <= set(range(80, 88)) | {123} and raw[352:] == np.asfortranarray(arr).tobytes(order="F")
    assert np.array_equal(read_nifti(str(tmp_path / "b.nii.gz")), arr)
    assert read_nifti_pixdim_mm(str(tmp_path / "b.nii.gz")) == pytest.approx((0.2, 0.3), rel=1e-7)
    assert read_nifti_pixdim_mm(str(tmp_path / "a.nii")) == (0.0, 0.0)


def test_converter_units_and_refusals():
    from tools.convert_camus import spacing_um
    assert spacing_um(0.2, 0.3, 90, 60, 32) == [844, 375]
    assert spacing_um(0.308, 0.154, 549, 778, 256) == [330, 936]
    for bad in ((0.0, 0.3), (0.2, -1.0), (math.nan, 0.3), (0.2, math.inf)):
        assert spacing_um(*bad, 90, 60, 32) is None
    assert spacing_um(0.2, 0.3, 90, 60, 1) is None and spacing_um(1e-6, 0.3, 90, 60, 32) is None      # above 4095, below 1


def test_spacing_from_the_nifti_header_to_the_table(tmp_path):
    """pixdim (0.2, 0.3) mm, native 60 wide x 90 high, --size 32: rows of 300 * 90 / 32 um, columns of 200 * 60 / 32 um."""
    from types import SimpleNamespace
    from gdkvm_amd.config import load_config
    from gdkvm_amd.data import CamusPng, NpzClips, SyntheticEchoClips, clip_spacing_table
    from tools.convert_camus import convert
    src, dst = tmp_path / "camus", tmp_path / "png"
    _camus_tree(src, (0.2, 0.3))
    logs = []
    assert convert(str(src), str(dst), size=32, frames=3, split="val", log=logs.append) == {"sequences": 2}
    for view in ("2CH", "4CH"):
        with open(dst / "val" / "patient0001" / view / "spacing.json") as f:
            assert json.load(f) == {"spacing_um": [844, 375], "native_hw": [90, 60]}
    assert [844, 375] == [int(np.rint(300 * 90 / 32)), int(np.rint(200 * 60 / 32))] and len(logs) == 1
    ds = CamusPng(str(dst), "val", 3)
    assert ds.spacing_um(0) == (844, 375) and ds.spacing_um(1) == (844, 375)
    x, y = ds[0]
    assert x.shape == (3, 3, 32, 32) and y.shape == (3, 32, 32)          # the samples stay (frames, target)
    cfg = load_config(None, [])
    assert cfg.data.spacing_um is None
    tab = clip_spacing_table(ds, cfg)
    assert tab.dtype.is_floating_point is False and str(tab.dtype) == "torch.int32" and tab.tolist() == [[844, 375], [844, 375]]
    # one sequence loses its file: no table without the fallback, the fallback for that clip alone with it
    os.remove(dst / "val" / "patient0001" / "4CH" / "spacing.json")
    assert ds.spacing_um(1) is None and clip_spacing_table(ds, cfg) is None
    with_fb = load_config(None, ["data.spacing_um=[330,468]"])
    assert with_fb.data.spacing_um == [330, 468] and clip_spacing_table(ds, with_fb).tolist() == [[844, 375], [330, 468]]
    # a file that holds no usable pair counts as no file
    with open(dst / "val" / "patient0001" / "4CH" / "spacing.json", "w") as f:
        json.dump({"spacing_um": [0, 375]}, f)
    assert ds.spacing_um(1) is None
    # a tree without pixdim: no file, one log line per sequence
    src2, dst2, logs2 = tmp_path / "camus2", tmp_path / "png2", []
    _camus_tree(src2, None)
    convert(str(src2), str(dst2), size=32, frames=3, split="val", log=logs2.append)
    assert not os.path.exists(dst2 / "val" / "patient0001" / "2CH" / "spacing.json") and sum("spacing" in l for l in logs2) == 2
    assert clip_spacing_table(CamusPng(str(dst2), "val", 3), cfg) is None
    # the other datasets: the synthetic one has none of its own, .npz clips an optional array
    syn = SyntheticEchoClips(3, 2, 16)
    assert syn.spacing_um(0) is None and clip_spacing_table(syn, cfg) is None and clip_spacing_table(syn, with_fb).tolist() == [[330, 468]] * 3
    (tmp_path / "npz" / "val").mkdir(parents=True)
    fr, mk = np.zeros((2, 8, 8), np.uint8), np.zeros((2, 8, 8), np.uint8)
    np.savez(tmp_path / "npz" / "val" / "a.npz", frames=fr, masks=mk, spacing_um=np.asarray([400, 500]))
    np.savez(tmp_path / "npz" / "val" / "b.npz", frames=fr, masks=mk)
    nz = NpzClips(str(tmp_path / "npz"), "val", 2)
    assert nz.spacing_um(0) == (400, 500) and nz.spacing_um(1) is None and clip_spacing_table(nz, cfg) is None
    assert clip_spacing_table(nz, with_fb).tolist() == [[400, 500], [330, 468]]
    assert clip_spacing_table(nz, SimpleNamespace(data=SimpleNamespace(spacing_um=[1, 4095]))).tolist() == [[400, 500], [1, 4095]]


def test_spacing_um_config_key():
    from gdkvm_amd.config import load_config
    path = os.path.join(ROOT, "config", "config_gdkvm_01.yaml")
    assert load_config(path).data.spacing_um is None and load_config(path, ["data.spacing_um=null"]).data.spacing_um is None
    assert load_config(path, ["data.spacing_um=[1,4095]"]).data.spacing_um == [1, 4095]
    for bad in ("[0,300]", "[300,4096]", "[300]", "[300,300,300]", "300", "[300.0,300]", "[true,300]", "[-1,5]", "abc"):
        with pytest.raises(ValueError, match="spacing_um"):
            load_config(path, [f"data.spacing_um={bad}"])


def test_the_header_and_ops_agree_on_the_constants():
    import re
    from gdkvm_amd import ops
    with open(os.path.join(ROOT, "include", "gdkvm.h")) as f:
        header = f.read()
    assert int(re.search(r"#define\s+GDKVM_SURFACE_MM_LDS_PIXELS\s+(\d+)", header).group(1)) == ops.SURFACE_MM_LDS_PIXELS == 144 * 128
    assert ops.SPACING_UM_MAX == P.UM_MAX == 4095
    for name in ("gdkvm_surface_distance_mm_workspace_bytes", "gdkvm_surface_distance_mm", "gdkvm_lv_measure_mm"):
        assert name in ops.SIGNATURES and re.search(r"\b" + name + r"\s*\(", header)
