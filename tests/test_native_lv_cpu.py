"""gdkvm_lv_measure_native without a device: tests/native_lv_reference.py (the definition in include/gdkvm.h for sides up to 2048) against
tests/spacing_reference.lv_measure_mm_ref word for word, against the prolate spheroid, and on the inputs that reach the header's integer
bounds (the reference asserts every bound on every input); the host path of ops.lv_measure_native against it; every refusal of the wrapper
and of the C entry, which answers before its first device call; the configuration key; ops.native_spacing_frames."""
import math
import os

import numpy as np
import pytest
import torch

from tests import native_lv_reference as R
from tests import spacing_reference as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = R.Q


def _blob(rng, h, w, p=0.4):
    return (rng.random((h, w)) < p).astype(np.uint8) + 2 * (rng.random((h, w)) < 0.1).astype(np.uint8)      # bytes 0..3: 1 is the class


def test_reference_equals_the_mm_reference_word_for_word():
    rng = np.random.default_rng(1)
    for h, w in ((64, 64), (33, 7), (1, 1), (1, 7), (7, 1), (40, 61)):
        m = _blob(rng, h, w)
        for ry, rx in ((300, 450), (1, 4095), (4095, 1), (4095, 4095), (1000, 1000)):
            for cls, D in ((1, 20), (1, 1), (2, 64), (3, 7)):
                a, b = R.measure(m, ry, rx, cls, D), P.lv_measure_mm_ref(m, ry, rx, cls, D)
                assert a["stats"] == b["stats"] and a["disks"] == b["disks"] and a["geom"] == b["geom"], (h, w, ry, rx, cls, D)
                rows = np.asarray(a["bands"], dtype=object)
                assert rows.shape == ((h + R.BAND_ROWS - 1) // R.BAND_ROWS, 8 + D)
                if a["stats"][0]:                             # the bands add up to the frame
                    assert [int(v) for v in rows[:, :6].sum(0)] == a["stats"][:6] and [int(v) for v in rows[:, 8:].sum(0)] == a["disks"]
                    assert min(rows[:, 6]) == a["stats"][8] and max(rows[:, 7]) == a["stats"][9]
                else:
                    assert not rows.any()


def test_band_rows_of_empty_bands_and_empty_frames():
    m = np.zeros((70, 9), np.uint8)
    m[3:9, 2:5] = 1
    m[66:, 1:8] = 1                                           # bands 0 and 2 occupied, band 1 empty
    r = R.measure(m, 300, 450)
    assert r["bands"][1] == [0] * 6 + [R.I64_MAX, R.I64_MIN] + [0] * 20 and r["bands"][0][0] == 18 and r["bands"][2][0] == 28
    assert R.measure(np.zeros((70, 9), np.uint8), 300, 450)["bands"] == [[0] * 28] * 3


def test_rasterised_ellipse_at_a_native_size_is_close_to_the_prolate_spheroid():
    """test_spacing_cpu's closed form (semi-axes 35 x 15 mm, tolerance 0.0075 of the volume) on a 1150 x 900 frame of 0.110 x 0.154 mm pixels"""
    ry, rx, la, sa = 110, 154, 35.0, 15.0
    want = 4.0 / 3.0 * math.pi * la * sa * sa / 1000
    yy, xx = np.mgrid[0:1150, 0:900].astype(np.float64)
    dy, dx = (yy - 574.5) * ry / 1000, (xx - 449.5) * rx / 1000
    for deg in (0, 30, 90):
        th = math.radians(deg)
        al, ac = dx * math.sin(th) + dy * math.cos(th), dx * math.cos(th) - dy * math.sin(th)
        m = ((al / la) ** 2 + (ac / sa) ** 2 <= 1.0).astype(np.uint8)
        res = R.measure(m, ry, rx)
        assert abs(res["geom"][1] - want) <= 0.0075 * want, (deg, res["geom"][1] / want)
        assert res["geom"][0] == pytest.approx(2 * la, rel=0.02)


def extreme_frames():
    """(name, frame, spacing): the inputs that reach the header's bounds -- the test of the device runs the same ones"""
    full = np.ones((2048, 2048), np.uint8)
    sides = np.zeros((2048, 2048), np.uint8)
    sides[:, :512] = 1
    sides[:, -512:] = 1
    diag = np.eye(2048, dtype=np.uint8)
    rng = np.random.default_rng(7)
    return [("full", full, (300, 450)), ("sides", sides, (450, 300)), ("diagonal", diag, (4095, 1)),
            ("2x2048", (rng.random((2, 2048)) < 0.5).astype(np.uint8), (1, 4095)),
            ("2048x2", (rng.random((2048, 2)) < 0.5).astype(np.uint8), (4095, 4095))]


def test_the_bounds_hold_on_the_extreme_inputs():
    for name, m, (ry, rx) in extreme_frames():
        for D in (20, 64) if name == "diagonal" else (20,):
            r = R.measure(m, ry, rx, 1, D)                    # (asserts |A|, |B|, |C| < 2^63, |t| < 2^50, W_j < 2^63, sum W_j = n D P1)
            n, sx, sxx = r["stats"][0], r["stats"][1], r["stats"][3]
            assert sum(r["disks"]) == n * D * n * r["stats"][11]
            if name == "full":
                A = n * sxx - sx * sx
                assert n == 1 << 22 and A == (1 << 44) * (2048 ** 2 - 1) // 12 and n * sxx >= 1 << 64       # the products do not fit 64 bits
                assert n * 2047 > 1 << 32                     # ... and n x does not fit 32
            if name == "diagonal":                            # the longest axis: 2048 pixels along the anisotropic diagonal
                assert r["geom"][0] == pytest.approx(2048 * math.hypot(4.095, 0.001), rel=1e-3)


def test_ops_host_path_equals_the_reference():
    from gdkvm_amd import ops
    rng = np.random.default_rng(3)
    sizes, T = [(47, 61), (5, 7), (65, 33), (1, 1)], 3
    clips = [np.stack([_blob(rng, h, w) for _ in range(T)]) for h, w in sizes]
    clips[1][1] = 0                                           # an empty frame
    clips[2][2, :33] = 0                                      # the class only in the last two bands
    sp = [(300, 450), (1, 4095), (4095, 1), (1000, 1000)]
    flat, sz = R.pack(clips)
    assert sz == sizes
    for cls, D in ((1, 20), (2, 1), (1, 64)):
        want = R.records(clips, sp, cls, D)
        got = ops.lv_measure_native(torch.from_numpy(flat), sizes, T, sp, cls=cls, disks=D, want_bands=True)
        assert [tuple(t.shape) for t in got] == [(4, T, 12), (4, T, D), (4, T, 6), (T * (2 + 1 + 3 + 1), 8 + D)]
        assert got[0].dtype == got[1].dtype == got[3].dtype == torch.int64 and got[2].dtype == torch.float64
        for g, w in zip(got, want):
            assert np.array_equal(g.numpy().view(np.int64), w.view(np.int64))
        three = ops.lv_measure_native(torch.from_numpy(flat), torch.tensor(sizes), T, torch.tensor(sp), cls=cls, disks=D)
        assert len(three) == 3 and all(torch.equal(a, b) for a, b in zip(three, got))


def test_ops_refusals_without_a_device():
    from gdkvm_amd import ops
    m = torch.zeros(2 * (30 + 21), dtype=torch.uint8)
    sizes, sp = [(5, 6), (7, 3)], [(300, 200), (100, 100)]
    f = ops.lv_measure_native
    assert [tuple(t.shape) for t in f(m, sizes, 2, sp)] == [(2, 2, 12), (2, 2, 20), (2, 2, 6)]
    for bad in ([(0, 6), (7, 3)], [(5, 6), (7, 2049)]):
        with pytest.raises(ops.GdkvmError, match="outside 1..2048"):
            f(m, bad, 2, sp)
    for bad in ([(0, 200), (100, 100)], [(300, 200), (100, 4096)]):
        with pytest.raises(ops.GdkvmError, match="outside 1..4095"):
            f(m, sizes, 2, bad)
    with pytest.raises(ops.GdkvmError, match="sizes must be host integers"):
        f(m, torch.tensor(sizes, device="meta"), 2, sp)
    with pytest.raises(ops.GdkvmError, match="spacing_um must be host integers"):
        f(m, sizes, 2, torch.tensor(sp, device="meta"))
    with pytest.raises(ops.GdkvmError, match="1 spacings for 2 clips"):
        f(m, sizes, 2, sp[:1])
    with pytest.raises(ops.GdkvmError, match="no pair of integers"):
        f(m, sizes, 2, [(300.0, 200), (100, 100)])
    with pytest.raises(ops.GdkvmError, match="mask must be a flat uint8 tensor of at least 102 bytes"):
        f(m[:-1], sizes, 2, sp)
    with pytest.raises(ops.GdkvmError, match="mask must be a flat uint8"):
        f(m.to(torch.int32), sizes, 2, sp)
    with pytest.raises(ops.GdkvmError, match="mask must be a flat uint8"):
        f(m.reshape(2, -1), sizes, 2, sp)
    for cls in (255, -1, True):
        with pytest.raises(ops.GdkvmError, match="cls"):
            f(m, sizes, 2, sp, cls=cls)
    for D in (0, 65, True, 2.0):
        with pytest.raises(ops.GdkvmError, match="disks"):
            f(m, sizes, 2, sp, disks=D)
    with pytest.raises(ops.GdkvmError, match="T = 0"):
        f(m, sizes, 0, sp)
    assert (ops.LV_NATIVE_BAND_ROWS, ops.LV_NATIVE_MAX_WG, ops.LV_NATIVE_CLIPS) == (32, 4096, 64) and R.BAND_ROWS == ops.LV_NATIVE_BAND_ROWS
    hdr = open(os.path.join(ROOT, "include", "gdkvm.h")).read()
    for name in ("BAND_ROWS", "MAX_WG", "CLIPS"):             # the header's macros are the module's constants
        assert f"#define GDKVM_LV_NATIVE_{name} {getattr(ops, 'LV_NATIVE_' + name)}\n" in hdr
    assert "gdkvm_lv_measure_native" in ops.SIGNATURES and "gdkvm_lv_measure_native_workspace_bytes" not in ops.SIGNATURES


def test_entry_refuses_bad_arguments_without_a_device():
    """The C entry validates everything before its first device call, so it answers on a machine without a GPU too."""
    from gdkvm_amd import ops
    lib = ops.load()
    sizes, sp = np.array([[5, 6], [70, 3]], np.int32), np.array([[300, 200], [100, 100]], np.int32)
    total, nbands, D = 2 * (30 + 210), 2 * (1 + 3), 20
    m = np.zeros(total, np.uint8)

    def aligned(words):
        buf = np.zeros(words + 2, np.int64)
        return buf, buf.ctypes.data + (-buf.ctypes.data) % 16

    keep, (st, dk, ge, bd) = zip(*(aligned(n) for n in (4 * 12, 4 * D, 4 * 6, nbands * (8 + D))))

    def call(mask=m.ctypes.data, sz=sizes, spc=sp, stats=st, disks=dk, geom=ge, bands=bd, nb=total, nbd=nbands, clips=2, T=2, cls=1, D=D):
        return lib.gdkvm_lv_measure_native(mask, sz.ctypes.data if sz is not None else None, spc.ctypes.data if spc is not None else None,
                                           stats, disks, geom, bands, nb, nbd, clips, T, cls, D, None)

    shape = [dict(clips=-1), dict(T=0), dict(D=0), dict(D=65), dict(sz=np.array([[5, 6], [0, 3]], np.int32)),
             dict(sz=np.array([[2049, 6], [70, 3]], np.int32)), dict(spc=np.array([[0, 200], [100, 100]], np.int32)),
             dict(spc=np.array([[300, 200], [100, 4096]], np.int32)), dict(nb=total - 1), dict(nbd=nbands - 1), dict(nbd=nbands + 1), dict(nbd=-1),
             dict(clips=1 << 16, T=1 << 15)]
    arg = [dict(cls=255), dict(cls=-1), dict(mask=None), dict(sz=None), dict(spc=None), dict(stats=None), dict(disks=None), dict(geom=None),
           dict(bands=None), dict(stats=st + 8), dict(disks=dk + 8), dict(geom=ge + 8), dict(bands=bd + 8)]
    for code, cases in ((-1, shape), (-6, arg)):              # GDKVM_ERR_SHAPE, GDKVM_ERR_ARG
        for kw in cases:
            assert call(**kw) == code, kw
            assert b"lv_measure_native" in lib.gdkvm_last_error(), kw
    assert call(clips=0) == 0 and call(clips=0, mask=None, bands=None, nbd=0) == 0


def test_native_lv_config_key():
    from gdkvm_amd.config import load_config
    path = os.path.join(ROOT, "config", "config_gdkvm_01.yaml")
    for cfg in (load_config(path), load_config(None, [])):
        assert cfg.data.native_lv is False
    cfg = load_config(path, ["data.native_eval=true", "data.native_lv=true"])
    assert cfg.data.native_lv is True and cfg.data.lv_class >= 0
    with pytest.raises(ValueError, match="data.native_lv needs data.native_eval: true and data.lv_class >= 0"):
        load_config(path, ["data.native_lv=true"])
    with pytest.raises(ValueError, match="data.native_lv needs data.native_eval: true and data.lv_class >= 0"):
        load_config(path, ["data.native_eval=true", "data.native_lv=true", "data.lv_class=-1"])
    for bad in ("1", "maybe", "2.5"):
        with pytest.raises(ValueError, match="native_lv"):
            load_config(path, ["data.native_eval=true", f"data.native_lv={bad}"])


def test_native_spacing_frames():
    from gdkvm_amd import ops
    sp = [(300, 450), (1, 4095)]
    for given in (sp, torch.tensor(sp, dtype=torch.int32), torch.tensor(sp, dtype=torch.int64)):
        t = ops.native_spacing_frames(given, 3, "cpu")
        assert t.dtype == torch.int32 and tuple(t.shape) == (2, 3, 2) and t.is_contiguous()
        assert t.tolist() == [[list(p)] * 3 for p in sp]
    with pytest.raises(ops.GdkvmError, match="outside 1..4095"):
        ops.native_spacing_frames([(300, 4096)], 3, "cpu")
    with pytest.raises(ops.GdkvmError, match="spacing_um must be host integers"):
        ops.native_spacing_frames(torch.tensor(sp, device="meta"), 3, "cpu")
    with pytest.raises(ops.GdkvmError, match="T = 0"):
        ops.native_spacing_frames(sp, 0, "cpu")
