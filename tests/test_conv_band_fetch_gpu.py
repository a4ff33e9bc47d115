"""The 3x3 convolutions stage their input halo band in LDS through a buffer descriptor whose range check supplies the zero padding
above and below a frame.  What such a range check can get wrong: a halo row that is the neighbouring frame's row in memory (it is in
range), memory in front of the first and behind the last frame, and an out-of-range lane that leaves its LDS slot as the previous
tile wrote it instead of zeroing it."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CL = dict(memory_format=torch.channels_last)

# (N, C, H, W, K, residual)
POISON_SHAPES = [(3, 256, 7, 7, 256, False),          # several frames per tile; the last group ragged under kernel 0 (2 + 1 frames)
                 (5, 64, 4, 4, 128, False),           # five frames in one tile
                 (7, 256, 7, 7, 256, False),          # ragged last group under both kernels (2 + 2 + 2 + 1 frames; 4 + 3)
                 (11, 64, 4, 4, 128, False),          # likewise (5 + 5 + 1; 9 + 2: the band of more frames does not fit the DMA pieces)
                 (3, 128, 14, 14, 128, False),                                # row tiles of 8 + 6
                 (3, 192, 28, 28, 64, False),
                 (3, 64, 28, 28, 64, False), (3, 64, 28, 28, 64, True),       # the 64 -> 64 kernel, one tile per row
                 (3, 64, 9, 11, 64, False), (3, 64, 9, 11, 64, True),
                 (2, 64, 30, 41, 64, False)]                                  # the 64 -> 64 kernel, two tiles per row (per-lane pointers)
CAT_SHAPES = [(2, 128, 64, 28, 28, 64), (3, 256, 128, 14, 14, 128)]           # (N, C1, C2, H, W, K)


def _layer(c, k, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    wt = (torch.randn(k, c, 3, 3, device="cuda", generator=g) / (9 * c) ** 0.5).bfloat16().contiguous(**CL)
    return wt, torch.randn(k, device="cuda", generator=g), g


def _guarded(t):
    """A channels_last copy of t that lies in the middle of a NaN-filled buffer, more than an image row of NaN on either side,
    16-byte aligned."""
    n, c, h, w = t.shape
    guard = (w + 2) * c + 8
    buf = torch.full((2 * guard + t.numel(),), float("nan"), dtype=t.dtype, device=t.device)
    view = buf[guard:guard + t.numel()].view(n, h, w, c).permute(0, 3, 1, 2)
    view.copy_(t)
    assert view.is_contiguous(**CL) and view.data_ptr() % 16 == 0 and torch.equal(view, t)
    return view


@pytest.mark.parametrize("kernel", [0, 7])      # by shape (the four-wave and the 64 -> 64 kernels); the eight-wave chunked kernel
@pytest.mark.parametrize("case", POISON_SHAPES)
def test_frame_independence_under_poison(hip, case, kernel):
    """Every frame but one is NaN: that frame's output is finite and bit-equal to the frame convolved alone."""
    n, c, h, w, k, with_res = case
    wt, b, g = _layer(c, k, sum(case[:5]))
    x = torch.randn(n, c, h, w, device="cuda", generator=g).bfloat16().contiguous(**CL)
    r = torch.randn(n, k, h, w, device="cuda", generator=g).bfloat16().contiguous(**CL) if with_res else None
    for keep in sorted({0, n // 2, n - 1}):
        xp = torch.full_like(x, float("nan"))
        xp[keep] = x[keep]
        rp = None
        if with_res:
            rp = torch.full_like(r, float("nan"))
            rp[keep] = r[keep]
        got = hip.conv_bias_act(xp, wt, b, rp, 1, 1, True, kernel)[keep]
        alone = hip.conv_bias_act(x[keep:keep + 1].contiguous(**CL), wt, b, r[keep:keep + 1].contiguous(**CL) if with_res else None,
                                  1, 1, True, kernel)[0]
        assert torch.isfinite(got.float()).all(), f"frame {keep}: non-finite output"
        assert torch.equal(got, alone), f"frame {keep}: differs from the frame alone"


@pytest.mark.parametrize("kernel", [0, 7])
@pytest.mark.parametrize("case", POISON_SHAPES)
def test_guarded_storage(hip, case, kernel):
    """The input lies between NaNs in memory: same result as on a tensor of its own."""
    n, c, h, w, k, with_res = case
    wt, b, g = _layer(c, k, 1 + sum(case[:5]))
    x = torch.randn(n, c, h, w, device="cuda", generator=g).bfloat16().contiguous(**CL)
    r = torch.randn(n, k, h, w, device="cuda", generator=g).bfloat16().contiguous(**CL) if with_res else None
    want = hip.conv_bias_act(x, wt, b, r, 1, 1, True, kernel)
    got = hip.conv_bias_act(_guarded(x), wt, b, r, 1, 1, True, kernel)
    assert torch.isfinite(got.float()).all() and torch.equal(got, want)


@pytest.mark.parametrize("kernel", [0, 7])
@pytest.mark.parametrize("case", CAT_SHAPES)
def test_guarded_storage_concatenated(hip, case, kernel):
    """conv_cat_bias_act with both inputs between NaNs in memory: same result as on tensors of their own."""
    n, c1, c2, h, w, k = case
    wt, b, g = _layer(c1 + c2, k, sum(case))
    x1 = torch.randn(n, c1, h, w, device="cuda", generator=g).bfloat16().contiguous(**CL)
    x2 = torch.randn(n, c2, h, w, device="cuda", generator=g).bfloat16().contiguous(**CL)
    want = hip.conv_cat_bias_act(x1, x2, wt, b, None, True, kernel)
    got = hip.conv_cat_bias_act(_guarded(x1), _guarded(x2), wt, b, None, True, kernel)
    assert torch.isfinite(got.float()).all() and torch.equal(got, want)
    assert torch.equal(want, hip.conv_bias_act(torch.cat([x1, x2], 1).contiguous(**CL), wt, b, None, 1, 1, True, kernel))


# More tiles than workgroups (grids of 512).  The 64 -> 64 kernel alternates two band buffers per TILE, so a buffer is written again by a
# workgroup's third tile: 150 frames x 7 row tiles = 1050 tiles, and tiles b, b + 1024 differ in their row tile (1024 = 2 mod 7): top-edge,
# interior and bottom-edge bands follow one another in one buffer.  The chunked kernel alternates per 64-channel CHUNK, so a 128-channel layer's
# second tile reuses both buffers; at 28 x 28 a frame is seven row tiles and tiles b, b + 512 differ by one row tile (80 frames: 560 tiles).
# (80 x 28 x 28 at 64 channels and 300 x 14 x 14 have more tiles than workgroups too, but each buffer sees one kind of band there.)
@pytest.mark.parametrize("case", [(80, 64, 28, 28, 64), (300, 128, 14, 14, 128), (150, 64, 28, 28, 64), (80, 128, 28, 28, 128)])
def test_reused_band_buffers(hip, case):
    """More tiles than workgroups: a workgroup writes an edge tile's band over an interior tile's and the other way round, so a lane
    that skipped its LDS write when out of range would leave the earlier tile's pixels where zeros belong."""
    n, c, h, w, k = case
    wt, b, g = _layer(c, k, sum(case))
    x = torch.randn(n, c, h, w, device="cuda", generator=g).bfloat16().contiguous(**CL)
    got = hip.conv_bias_act(x, wt, b, None, 1, 1, False, 0)
    want = torch.nn.functional.conv2d(x.double(), wt.double(), b.double(), 1, 1)
    err = (got.double() - want).abs().max().item()
    bound = 2.0 ** -7 * max(1.0, want.abs().max().item())
    print(f"max |got - want| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
