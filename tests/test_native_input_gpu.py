"""gdkvm_frames_from_native on the device against tests/native_input_reference.py, bit for bit, in its three output dtypes, and
predict.segment_native against the composition of its parts.  The shapes sit where the kernel can go wrong rather than at the workload's
size: odd h0 w0 (every later frame and clip starts at another alignment mod 16), enlarging and reducing ratios that are no whole number,
single pixels, the identity, many native rows or columns per grid pixel (columns and grid rows cut into parts, bands on both sides of the
accumulator budget), more native rows than one chunk holds, the 32-bit end of the numerator's range, and clip counts past one launch."""
import os
import re

import numpy as np
import pytest
import torch

from tests import native_input_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HDR = open(os.path.join(ROOT, "include", "gdkvm.h")).read()
_define = lambda name: int(re.search(r"#define GDKVM_FRAMES_FROM_NATIVE_" + name + r" (\d+)", _HDR).group(1))
CHUNK_BYTES, ACC_WORDS, PART, CLIPS = _define("CHUNK_BYTES"), _define("ACC_WORDS"), _define("PART"), _define("CLIPS")
ERR_SHAPE = int(re.search(r"GDKVM_ERR_SHAPE = (-?\d+)", _HDR).group(1))
DTYPES = (torch.uint8, torch.float32, torch.bfloat16)


def _same(out, ref):
    """the device tensor `out` against the reference bytes `ref` [clips, T, C, H, W], in out's dtype, bit for bit"""
    assert tuple(out.shape) == ref.shape
    if out.dtype == torch.uint8:
        return np.array_equal(out.cpu().numpy(), ref)
    if out.dtype == torch.float32:
        return np.array_equal(out.cpu().numpy().view(np.uint32), R.to_float32(ref).view(np.uint32))
    return np.array_equal(out.view(torch.int16).cpu().numpy().view(np.uint16), R.to_bf16_bits(ref))


def _check(hip, flat, sizes, T, grid, C, dtypes=DTYPES):
    ref, offs = R.frames_from_native(flat, sizes, T, grid[0], grid[1], C)
    dflat = torch.from_numpy(flat).cuda()
    for dt in dtypes:
        out, o2 = hip.frames_from_native(dflat, sizes, T, grid=grid, channels=C, dtype=dt)
        assert o2 == offs and out.dtype == dt and _same(out, ref), (sizes, T, grid, C, dt)
    return ref


@pytest.fixture(scope="module")
def ragged():
    """7 x 5 and 5 x 7, 1 x 1, 3 x 3, 33 x 17, 64 x 64, 97 x 130 at T = 3: odd sizes, so frames start at every alignment mod 16"""
    rng = np.random.default_rng(0)
    clips = [rng.integers(0, 256, (3, h0, w0), dtype=np.uint8) for h0, w0 in ((7, 5), (5, 7), (1, 1), (3, 3), (33, 17), (64, 64), (97, 130))]
    flat, sizes = R.pack(clips)
    starts = {(off + t * h0 * w0) % 16 for off, (h0, w0) in zip(np.cumsum([0] + [3 * h * w for h, w in sizes[:-1]]), sizes) for t in range(3)}
    assert len(starts) >= 8
    flat.setflags(write=False)
    return flat, sizes


@pytest.mark.parametrize("grid", [(4, 3), (8, 8), (64, 64)], ids=lambda g: "to_%dx%d" % g)
@pytest.mark.parametrize("C", [1, 3])
def test_ragged_batch_matches_the_restatement(hip, ragged, grid, C):
    flat, sizes = ragged
    ref = _check(hip, flat, sizes, 3, grid, C)
    if grid == (64, 64):                                       # 64 x 64 onto a 64 x 64 grid is the identity, in every plane
        off = sum(3 * h * w for h, w in sizes[:5])
        assert np.array_equal(ref[5], np.broadcast_to(flat[off:off + 3 * 64 * 64].reshape(3, 1, 64, 64), (3, C, 64, 64)))


def test_out_at_an_aligned_and_at_an_offset_base(hip, ragged):
    """out is promised 16-byte aligned: an aligned slice of a larger buffer is written (and nothing around it), an offset one is refused"""
    flat, sizes = ragged
    ref, _ = R.frames_from_native(flat, sizes, 3, 8, 8, 3)
    dflat = torch.from_numpy(flat).cuda()
    n = ref.size
    for dt in DTYPES:
        per = 16 // torch.empty(0, dtype=dt).element_size()
        buf = torch.zeros(n + 4 * per, dtype=dt, device="cuda")
        assert buf.data_ptr() % 16 == 0
        view = buf[per:per + n].view(ref.shape)
        out, _ = hip.frames_from_native(dflat, sizes, 3, grid=(8, 8), channels=3, dtype=dt, out=view)
        assert out is view and _same(view, ref)
        assert not buf[:per].any() and not buf[per + n:].any()
        with pytest.raises(hip.GdkvmError, match="frames_from_native: out must be 16-byte aligned"):
            hip.frames_from_native(dflat, sizes, 3, grid=(8, 8), channels=3, dtype=dt, out=buf[1:1 + n].view(ref.shape))
    # the C entry refuses it too, before any launch
    lib = hip.load()
    host = np.array(sizes, np.int32)
    buf = torch.zeros(n + 32, dtype=torch.uint8, device="cuda")
    rc = lib.gdkvm_frames_from_native(dflat.data_ptr(), host.ctypes.data, buf.data_ptr() + 5, flat.size, None, 0, len(sizes), 3, 3, 8, 8, 0, None)
    assert rc == ERR_SHAPE and b"16-byte aligned" in lib.gdkvm_last_error()
    torch.cuda.synchronize()
    assert not buf.any()


@pytest.mark.parametrize("case", [((2048, 3), (5, 2)), ((3, 2048), (2, 5))], ids=["tall_narrow", "wide_flat"])
def test_many_native_rows_or_columns_per_grid_pixel(hip, case):
    """2048 x 3 to 5 x 2: 411 native rows per grid row (> PART: rows cut into 32 parts), two bands of 4 and 1 grid rows (a band is the
    grid rows that one chunk's native rows are sure to cover), an odd native row length.  3 x 2048 to 2 x 5: 411 native columns per grid column
    (> PART: columns cut into parts), one grid row per band."""
    (h0, w0), grid = case
    assert max(-(-h0 // grid[0]), -(-w0 // grid[1])) > PART and ACC_WORDS >= 1024
    rng = np.random.default_rng(1)
    flat, sizes = R.pack([rng.integers(0, 256, (2, h0, w0), dtype=np.uint8)])
    for C in (1, 3):
        _check(hip, flat, sizes, 2, grid, C)


def test_largest_frame_and_the_32_bit_bound(hip):
    """One frame of 2048 x 2048: all 255 to 1 x 1 (2 N + h0 w0 = 511 * 2^22, the top of the range) and to 16 x 16; random bytes to 16 x 16.
    A grid row covers 128 native rows of 2048 bytes: many chunks per band."""
    assert 128 * 2048 > CHUNK_BYTES
    full = np.full((1, 2048, 2048), 255, np.uint8)
    flat, sizes = R.pack([full])
    for grid in ((1, 1), (16, 16)):
        ref = _check(hip, flat, sizes, 1, grid, 3)
        assert (ref == 255).all()
    flat, sizes = R.pack([np.random.default_rng(2).integers(0, 256, (1, 2048, 2048), dtype=np.uint8)])
    _check(hip, flat, sizes, 1, (16, 16), 3)


@pytest.mark.parametrize("grid", [(16, 16), (256, 256)], ids=lambda g: "to_%dx%d" % g)
def test_the_workload_s_ratio_at_one_frame(hip, grid):
    flat, sizes = R.pack([np.random.default_rng(3).integers(0, 256, (1, 549, 778), dtype=np.uint8)])
    _check(hip, flat, sizes, 1, grid, 3)


def test_more_clips_than_one_launch_carries_the_offsets(hip):
    rng = np.random.default_rng(4)
    flat, sizes = R.pack([rng.integers(0, 256, (2, 5, 4), dtype=np.uint8) for _ in range(CLIPS + 1)])
    _check(hip, flat, sizes, 2, (2, 2), 3)
    _check(hip, flat, sizes, 2, (2, 2), 1, dtypes=(torch.bfloat16,))


def test_two_calls_are_equal_and_no_clips_is_no_launch(hip, ragged):
    flat, sizes = ragged
    dflat = torch.from_numpy(flat).cuda()
    for dt in DTYPES:
        a = hip.frames_from_native(dflat, sizes, 3, grid=(8, 8), dtype=dt)[0]
        b = hip.frames_from_native(dflat, sizes, 3, grid=(8, 8), dtype=dt)[0]
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    out, offs = hip.frames_from_native(torch.zeros(0, dtype=torch.uint8, device="cuda"), [], 2, grid=(4, 4))
    assert tuple(out.shape) == (0, 2, 3, 4, 4) and offs == []
    with pytest.raises(hip.GdkvmError, match="sizes must be host integers"):
        hip.frames_from_native(dflat, torch.tensor(sizes, device="cuda"), 3, grid=(8, 8))
    with pytest.raises(hip.GdkvmError, match="out must not overlap flat"):
        hip.frames_from_native(dflat, [(8, 8)], 1, grid=(8, 8), channels=1, dtype=torch.uint8, out=dflat[:64].view(1, 1, 1, 8, 8))


def test_float_forms_are_the_prefetcher_s_cast_of_the_bytes(hip, ragged):
    """frames_from_native(dtype=bf16 / fp32) == DevicePrefetcher._convert's expression on the uint8 result: torch.mul(bytes, 1 / 255, out=...)"""
    flat, sizes = ragged
    dflat = torch.from_numpy(flat).cuda()
    q = hip.frames_from_native(dflat, sizes, 3, grid=(64, 64), dtype=torch.uint8)[0]
    for dt in (torch.bfloat16, torch.float32):
        want = torch.empty(q.shape, dtype=dt, device="cuda")
        torch.mul(q, 1.0 / 255.0, out=want)
        got = hip.frames_from_native(dflat, sizes, 3, grid=(64, 64), dtype=dt)[0]
        assert torch.equal(got, want)


def test_segment_native_is_the_composition_of_its_parts(hip):
    """predict.segment_native with a small random model on three ragged clips: its native masks are the reference rule -> the model through
    SegmentRunner -> the configured post-processing -> ops.mask_to_native, and its EF is ops.lv_ef of ops.lv_measure of the grid masks.
    This pins the wiring, not the network."""
    from gdkvm_amd.config import load_config
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    from gdkvm_amd.pipeline import SegmentRunner
    from gdkvm_amd.predict import grid_spacing_um, segment_native
    torch.manual_seed(0)
    cfg = load_config(None, ["data.size=64", "data.lv_fill_holes=4", "data.temporal_vote=1", "data.lv_beats=true", "data.beat_distance=1"])
    model = GDKVM(GDKVMConfig(num_classes=cfg.data.num_classes, widths=(16, 32, 64), pixel_dim=64, value_dim=32)).eval()
    with torch.no_grad():
        model.decoder.head.bias[1] += 0.05                    # random init is one class everywhere; tilt it so masks are mixed
    model = model.fuse_for_inference().cuda().to(torch.bfloat16).to(memory_format=torch.channels_last)
    rng = np.random.default_rng(5)
    sizes = [(97, 130), (64, 64), (33, 17)]
    clips = [rng.integers(0, 256, (3, h0, w0), dtype=np.uint8) for h0, w0 in sizes]
    spacing = [(300.0, 250.0), None, (1.0e6, 300.0)]          # usable, absent, out of range on the grid
    res = segment_native(model, cfg, [torch.from_numpy(c) for c in clips], spacing)
    # the parts, one by one
    flat, _ = R.pack(clips)
    ref = R.frames_from_native(flat, sizes, 3, 64, 64, 3)[0]
    frames = torch.from_numpy(R.to_bf16_bits(ref).view(np.int16)).cuda().view(torch.bfloat16)
    assert torch.equal(res["frames"], frames)
    mask, _ = SegmentRunner(model)(frames, None)
    mask, _, _ = hip.temporal_vote(mask, cfg.data.num_classes, 1)
    mask, _ = hip.fill_holes(mask, cls=1, connectivity=4, max_area=0)
    assert torch.equal(res["grid_mask"], mask)
    native, _, offs = hip.mask_to_native(mask, sizes, cfg.data.num_classes)
    rep = res["report"]
    assert rep["clips"] == 3 and rep["frames"] == 3 and rep["grid"] == [64, 64] and res["sizes"] == sizes
    stats, _, geom = hip.lv_measure(mask, cls=1)
    idx, val = hip.lv_ef(geom[..., 1].contiguous(), stats[..., 0].contiguous())
    for b, (h0, w0) in enumerate(sizes):
        m = res["masks"][b]
        assert m.dtype == torch.uint8 and tuple(m.shape) == (3, h0, w0)
        assert torch.equal(m, native[offs[b]:offs[b] + 3 * h0 * w0].view(3, h0, w0))
        pc = rep["per_clip"][b]
        assert pc["native_hw"] == [h0, w0] and {"lv", "beats", "temporal_vote", "fill_holes"} <= set(pc)
        assert pc["lv"]["ef"] == round(float(val[b, 2]), 5) and pc["lv"]["edv_px3"] == round(float(val[b, 0]), 5)
        assert [pc["lv"]["ed_frame"], pc["lv"]["es_frame"], pc["lv"]["valid_frames"]] == idx[b].tolist()
    g0 = grid_spacing_um(spacing[0], 97, 130, 64, 64)
    assert rep["per_clip"][0]["lv_mm"]["grid_spacing_um"] == list(g0)
    q_stats, _, q_geom = hip.lv_measure_mm(mask[:1], torch.tensor([[list(g0)]], dtype=torch.int32), cls=1)
    _, m_val = hip.lv_ef(q_geom[..., 1].contiguous(), q_stats[..., 0].contiguous())
    assert rep["per_clip"][0]["lv_mm"]["edv_ml"] == round(float(m_val[0, 0]), 5)
    assert "lv_mm" not in rep["per_clip"][1] and rep["per_clip"][1]["lv_mm_omitted"] == "no spacing"
    assert "lv_mm" not in rep["per_clip"][2] and "outside 1..4095" in rep["per_clip"][2]["lv_mm_omitted"]
