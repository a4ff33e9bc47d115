"""The persistent stem and 64 -> 64 convolution kernels request a tile's operands a tile ahead (the stem's look-ahead registers, the
64 -> 64 kernel's residual vectors and its LDS band) and wait for them under counted waits.  A wrong count faults nothing: it multiplies
stale or half-landed operands.  So every frame here carries values of its own, a workgroup walks at least three tiles (both band buffers
and the look-ahead registers are reused) and the checks are exact: against a form of the same call that has no loop-carried state, and
against fp64 at the neighbouring tests' bounds."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CL = dict(memory_format=torch.channels_last)


def _guarded_flat(t, guard):
    """(buffer, view): a copy of t's storage in the middle of a NaN-filled buffer, `guard` elements of NaN on either side (a multiple of
    8: the view stays 16-byte aligned)."""
    flat = t.permute(0, 2, 3, 1).reshape(-1) if t.is_contiguous(**CL) and not t.is_contiguous() else t.reshape(-1)
    buf = torch.full((2 * guard + flat.numel(),), float("nan"), dtype=t.dtype, device=t.device)
    buf[guard:guard + flat.numel()] = flat
    return buf, buf[guard:guard + flat.numel()]


# ---- the stem ---------------------------------------------------------------------------------------------------------------------------

# (frames, channels, H, W).  16 x 16 frames are one tile each: 770 = 3 x 256 + 2 tiles on 256 workgroups (three tiles each, two do four: the
# last look-ahead is skipped at different tiles); 5 frames: fewer tiles than workgroups, the loop body runs once with no look-ahead;
# 36 x 120: Hs x Ws = 18 x 60 -> pooled 9 x 30, tiles of 4 x 28: the last row tile and the second column tile ragged, six tiles per frame
STEM_CASES = [(770, 3, 16, 16), (5, 3, 16, 16), (40, 1, 36, 120), (40, 3, 36, 120), (40, 4, 36, 120)]


def _stem_inputs(case):
    n, c, hh, ww = case
    g = torch.Generator(device="cuda").manual_seed(sum(case))
    x = torch.randn(n, c, hh, ww, device="cuda", generator=g).bfloat16()
    w = (torch.randn(64, 16, 4, 4, device="cuda", generator=g) / 16).bfloat16().contiguous(**CL)
    return x, w, torch.randn(64, device="cuda", generator=g)


def _stem_check(hip, x, w, b, one):
    xs = hip.stem_s2d(x, 16)
    two = hip.stem_conv_pool(xs, w, b)
    assert one.shape == two.shape and torch.equal(one, two), "differs from stem_s2d + stem_conv_pool"
    hs, ws = xs.shape[2:]
    conv = torch.nn.functional.conv2d(xs.double(), w.double(), b.double(), 1, 2)[:, :, :hs, :ws]
    want = torch.nn.functional.max_pool2d(conv.relu().bfloat16().double(), 3, 2, 1)      # (test_stem_conv_pool_in_one_kernel's restatement)
    err, bound = (one.double() - want).abs().max().item(), 2.0 ** -7 * max(1.0, want.abs().max().item())
    print(f"max |got - want| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("case", STEM_CASES)
def test_stem_look_ahead(hip, case):
    """gdkvm_stem_conv_pool_nchw over several tiles per workgroup == gdkvm_stem_s2d + gdkvm_stem_conv_pool bit for bit, and right
    against fp64."""
    x, w, b = _stem_inputs(case)
    _stem_check(hip, x, w, b, hip.stem_conv_pool_nchw(x, w, b))


def test_stem_look_ahead_in_guarded_storage(hip):
    """The frames lie between NaNs in memory: no clamped or out-of-range slot of a band leaks a neighbour's value."""
    x, w, b = _stem_inputs(STEM_CASES[0])
    _, view = _guarded_flat(x, 4096)
    xg = view.view(x.shape)
    assert xg.is_contiguous() and xg.data_ptr() % 16 == 0 and torch.equal(xg, x)
    one = hip.stem_conv_pool_nchw(xg, w, b)
    assert torch.isfinite(one.float()).all()
    _stem_check(hip, x, w, b, one)


def test_training_stem_look_ahead(hip):
    """The convolution-only form of the same kernel (stem_conv), more tiles than workgroups: conv2d(stride 2, padding 3) in fp64 on the
    bf16-rounded operands, at test_training_stem_convolution_on_the_stem_kernel's bound."""
    g = torch.Generator(device="cuda").manual_seed(300)
    x = torch.randn(300, 3, 16, 16, device="cuda", generator=g).bfloat16()
    w = torch.randn(64, 3, 7, 7, device="cuda", generator=g) / (49 * 3) ** 0.5
    y = hip.stem_conv(x, w)
    ref = torch.nn.functional.conv2d(x.double(), w.bfloat16().double(), None, 2, 3)
    assert y.shape == ref.shape and y.dtype == torch.bfloat16 and y.is_contiguous(**CL)
    err, bound = (y.double() - ref).abs().max().item(), 2.0 ** -8 * max(1.0, ref.abs().max().item())
    print(f"max |got - want| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


# ---- the 64 -> 64 convolution ---------------------------------------------------------------------------------------------------------------

# [N, 64, H, W] on 512 workgroups.  1540 x 4 x 16: one tile per frame, three tiles per workgroup and four left over, tile width 16;
# 770 x 8 x 28: the shipped width 28, two row tiles per frame; 400 x 6 x 32: width 32, the last row tile's rows 6, 7 past the frame;
# 200 x 8 x 40: two tiles per row (the per-lane pointer form); 3 x 28 x 28: fewer tiles than workgroups
C64_SHAPES = [(1540, 4, 16), (770, 8, 28), (400, 6, 32), (200, 8, 40), (3, 28, 28)]
C64 = 4                                                     # gdkvm_conv_bias_act's kernel selector: the 64 -> 64 kernel
_c64_cache = {}


def _c64_inputs(shape):
    """Inputs and the fp64 convolution (bias included, no residual, no ReLU) of a shape, computed once and left unchanged."""
    if shape not in _c64_cache:
        n, h, w = shape
        g = torch.Generator(device="cuda").manual_seed(sum(shape))
        wt = (torch.randn(64, 64, 3, 3, device="cuda", generator=g) / (9 * 64) ** 0.5).bfloat16().contiguous(**CL)
        b = torch.randn(64, device="cuda", generator=g)
        x = torch.randn(n, 64, h, w, device="cuda", generator=g).bfloat16().contiguous(**CL)
        r = torch.randn(n, 64, h, w, device="cuda", generator=g).bfloat16().contiguous(**CL)
        ref = torch.nn.functional.conv2d(x.double(), wt.double(), b.double(), 1, 1)
        _c64_cache[shape] = (x, r, wt, b, ref)
    return _c64_cache[shape]


def _c64_reference(shape, with_res, relu):
    x, r, wt, b, ref = _c64_inputs(shape)
    want = ref + r.double() if with_res else ref
    return want.relu() if relu else want


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("shape", C64_SHAPES)
def test_c64_batched_equals_frame_by_frame(hip, shape, with_res, relu):
    """The batched call (several tiles per workgroup) == the same frames one per call (one tile per workgroup: no loop carry, no reused
    buffer) bit for bit, plain and packed weights; and right against fp64 at test_conv_with_fused_epilogue's bound."""
    x, r, wt, b, _ = _c64_inputs(shape)
    res = r if with_res else None
    got = hip.conv_bias_act(x, wt, b, res, 1, 1, relu, C64)
    assert torch.equal(got, hip.conv_bias_act(x, wt, b, res, 1, 1, relu, C64, hip.conv3x3_pack_weights(wt))), "packed weights differ"
    alone = torch.empty_like(got)
    for i in range(shape[0]):
        alone[i:i + 1] = hip.conv_bias_act(x[i:i + 1], wt, b, r[i:i + 1] if with_res else None, 1, 1, relu, C64)
    bad = (got.view(torch.int16) != alone.view(torch.int16)).flatten(1).any(1).nonzero().flatten().tolist()
    assert not bad, f"{len(bad)} frames differ from the frame alone, the first: {bad[:8]}"
    want = _c64_reference(shape, with_res, relu)
    err, bound = (got.double() - want).abs().max().item(), 2.0 ** -7 * max(1.0, want.abs().max().item())
    print(f"max |got - want| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("with_res", [False, True])
def test_c64_in_guarded_storage(hip, with_res, relu):
    """Input, residual and output each between NaNs in memory (through the C ABI: the output buffer is the test's): the same bits as on
    tensors of their own, and every NaN around the output still in place."""
    shape = C64_SHAPES[1]
    n, h, w = shape
    x, r, wt, b, _ = _c64_inputs(shape)
    want = hip.conv_bias_act(x, wt, b, r if with_res else None, 1, 1, relu, C64)
    guard = (w + 2) * 64 + 8
    _, xv = _guarded_flat(x, guard)
    _, rv = _guarded_flat(r, guard)
    ybuf = torch.full((2 * guard + x.numel(),), float("nan"), dtype=torch.bfloat16, device="cuda")
    yv = ybuf[guard:guard + x.numel()]
    assert xv.data_ptr() % 16 == 0 and rv.data_ptr() % 16 == 0 and yv.data_ptr() % 16 == 0
    lib = hip.load()
    rc = lib.gdkvm_conv_bias_act(xv.data_ptr(), wt.data_ptr(), b.data_ptr(), rv.data_ptr() if with_res else None, yv.data_ptr(), n, 64, h, w, 64, 3, 3,
                                 1, 1, int(relu), C64, hip.BF16, hip._stream(x.device))
    assert rc == 0
    got = yv.view(n, h, w, 64).permute(0, 3, 1, 2)
    assert torch.isfinite(got.float()).all() and torch.equal(got, want)
    assert torch.isnan(ybuf[:guard]).all() and torch.isnan(ybuf[guard + x.numel():]).all(), "a store landed outside the output"
