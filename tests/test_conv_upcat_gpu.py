"""gdkvm_conv_upcat_bias_act: the decoder's conv(cat(upsample2x(lo), x2)) with the enlarged feature built inside the convolution's LDS band.
Everything here is bit for bit against the two-launch path it replaces -- ops.upsample_bilinear (gdkvm_upsample_cat's 2x kernel) followed
by ops.conv_cat_bias_act on the same packed weights: the op on the shapes that reach every branch of the band logic, the band's edges
tap by tap, workgroups that take several tiles, and the fused inference model with GDKVM_UPCAT_FUSED=1 against =0."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

CL = dict(memory_format=torch.channels_last)

# (N, hl, wl): lo [N, C1, hl, wl] -> a map of 2 hl x 2 wl
SHAPES = [(5, 4, 4),        # 8 x 8: one frame per tile under the four-wave forms, whole frames with their own zero halo rows
          (5, 3, 3),        # 6 x 6: three frames per tile, the last group ragged (3 + 2), zero halo rows BETWEEN the frames of a band
          (3, 7, 7),        # 14 x 14: two row tiles per frame (8 + 6 rows), the second starting inside the frame
          (2, 14, 14),      # 28 x 28: 4-row tiles, 30-pixel band rows
          (1, 16, 16)]      # 32 x 32: a row width that is a multiple of 16


def _rand(g, *shape):
    return torch.randn(*shape, device="cuda", generator=g).bfloat16().contiguous(**CL)


def _two_launch(hip, lo, x2, wt, b, res, relu, packed):
    return hip.conv_cat_bias_act(hip.upsample_bilinear(lo, x2.shape[2:]), x2, wt, b, res, relu, 0, packed)


@pytest.mark.parametrize("k", [128, 64])                   # the <4, 2> and the <2, 2> form
@pytest.mark.parametrize("shape", SHAPES)
def test_op_equals_the_two_launch_path(hip, shape, k):
    """Random bf16 data; C1 = 64, 128, 256 (one, two and four consecutive enlarged chunks: the staging area is reused), C2 = 64, 128,
    ReLU on and off, with and without a residual."""
    n, hl, wl = shape
    g = torch.Generator(device="cuda").manual_seed(1000 * hl + 10 * n + k)
    for c1 in (64, 128, 256):
        lo = _rand(g, n, c1, hl, wl)
        for c2 in (64, 128):
            x2 = _rand(g, n, c2, 2 * hl, 2 * wl)
            wt = (torch.randn(k, c1 + c2, 3, 3, device="cuda", generator=g) / (9 * (c1 + c2)) ** 0.5).bfloat16().contiguous(**CL)
            b = torch.randn(k, device="cuda", generator=g)
            res = _rand(g, n, k, 2 * hl, 2 * wl)
            packed = hip.conv3x3_pack_weights(wt)
            for relu in (True, False):
                for r in (None, res):
                    want = _two_launch(hip, lo, x2, wt, b, r, relu, packed)
                    got = hip.conv_upcat_bias_act(lo, x2, wt, b, r, relu, packed)
                    assert torch.isfinite(got.float()).all()
                    assert torch.equal(got, want), (shape, k, c1, c2, relu, r is not None)
    assert torch.equal(hip.conv_upcat_bias_act(lo, x2, wt, b), _two_launch(hip, lo, x2, wt, b, None, True, packed))     # (packs the weights itself)


@pytest.mark.parametrize("k", [128, 64])
@pytest.mark.parametrize("shape", SHAPES)
def test_band_edges_tap_by_tap(hip, shape, k):
    """x2 = 0 and weights that are 1 on ONE tap (of enlarged channel j for output channel j) and 0 elsewhere: the output is the band
    itself, shifted by the tap.  With lo = 1 a halo pixel that holds a clamped value where the convolution's zero padding belongs is a
    non-zero border row or column; with random lo every interpolated value is compared directly, before any sum blurs it."""
    n, hl, wl = shape
    c1, c2 = 128, 64
    g = torch.Generator(device="cuda").manual_seed(77 + hl)
    x2 = torch.zeros(n, c2, 2 * hl, 2 * wl, device="cuda", dtype=torch.bfloat16).contiguous(**CL)
    b = torch.zeros(k, device="cuda")
    for lo in (torch.ones(n, c1, hl, wl, device="cuda", dtype=torch.bfloat16).contiguous(**CL), _rand(g, n, c1, hl, wl)):
        for tap in range(9):
            wt = torch.zeros(k, c1 + c2, 3, 3, device="cuda", dtype=torch.bfloat16)
            wt[torch.arange(k), torch.arange(k) % c1, tap // 3, tap % 3] = 1
            wt = wt.contiguous(**CL)
            packed = hip.conv3x3_pack_weights(wt)
            want = _two_launch(hip, lo, x2, wt, b, None, False, packed)
            got = hip.conv_upcat_bias_act(lo, x2, wt, b, None, False, packed)
            assert torch.equal(got, want), (shape, k, tap)
            if tap == 4:                                    # the centre tap: the enlargement itself
                assert torch.equal(got[:, :min(k, c1)], hip.upsample_bilinear(lo, x2.shape[2:])[:, :min(k, c1)])


@pytest.mark.parametrize("case", [(40, 128), (300, 128), (300, 64)])       # (N, K)
def test_workgroups_that_take_several_tiles(hip, case):
    """7 x 7 -> 14 x 14 through the op's ordinary path: 40 frames (80 tiles), and 300 frames -- 600 tiles on a grid capped at 512
    workgroups, so that a workgroup's second tile reuses the band buffers, the staging area and the weight ring of its first."""
    n, k = case
    g = torch.Generator(device="cuda").manual_seed(n + k)
    lo, x2 = _rand(g, n, 128, 7, 7), _rand(g, n, 64, 14, 14)
    wt = (torch.randn(k, 192, 3, 3, device="cuda", generator=g) / 192 ** 0.5 / 3).bfloat16().contiguous(**CL)
    b = torch.randn(k, device="cuda", generator=g)
    packed = hip.conv3x3_pack_weights(wt)
    assert torch.equal(hip.conv_upcat_bias_act(lo, x2, wt, b, None, True, packed), _two_launch(hip, lo, x2, wt, b, None, True, packed))


def _segment_with_feature(model, run):
    """run() with the stride-4 decoder feature (what segment() hands to the mask kernel) recorded."""
    seen = []
    h = model.decoder.register_forward_hook(lambda mod, args, out: seen.append(out))
    try:
        result = run()
    finally:
        h.remove()
    return result, seen


@pytest.mark.parametrize("side", [32, 112])                # 2 x 2 -> 4 x 4 -> 8 x 8 (seven and one frames per tile) and 7 -> 14 -> 28
def test_fused_model_with_and_without_the_switch(hip, side, monkeypatch):
    """The fused bf16 inference build, default widths, one clip of 2 frames: segment()'s masks and the decoder feature behind them are the
    same bits with GDKVM_UPCAT_FUSED=1 and =0, eagerly and through graphed_segment."""
    from gdkvm_amd.model import GDKVM, GDKVMConfig, HeadFeature
    torch.manual_seed(side)
    model = GDKVM(GDKVMConfig()).eval().fuse_for_inference().cuda().to(torch.bfloat16).to(memory_format=torch.channels_last)
    frames = torch.rand(1, 2, 3, side, side, device="cuda").bfloat16()
    fresh = torch.rand(1, 2, 3, side, side, device="cuda").bfloat16()
    out = {}
    with torch.no_grad():
        for flag in ("1", "0"):
            monkeypatch.setenv("GDKVM_UPCAT_FUSED", flag)
            (masks, _), seen = _segment_with_feature(model, lambda: model.segment(frames))
            assert len(seen) == 1 and isinstance(seen[0], HeadFeature)
            graph, gseen = _segment_with_feature(model, lambda: model.graphed_segment(frames.clone()))
            gm = graph(fresh)[0].clone()
            torch.cuda.synchronize()
            out[flag] = (masks.clone(), seen[0].feature.clone(), graph(frames)[0].clone(), gm, gseen[-1].feature.clone())
    for a, b_ in zip(out["1"], out["0"]):
        assert torch.equal(a, b_)
    assert torch.equal(out["1"][0], out["1"][2])            # the graph replays the eager call


def test_the_switch_selects_the_kernel(hip, monkeypatch):
    """UpBlock reaches the fused entry exactly when it is served and switched on (a refusal of the entry would otherwise go unnoticed
    behind the two-launch path)."""
    from gdkvm_amd import ops
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    torch.manual_seed(5)
    model = GDKVM(GDKVMConfig()).eval().fuse_for_inference().cuda().to(torch.bfloat16).to(memory_format=torch.channels_last)
    frames = torch.rand(1, 2, 3, 112, 112, device="cuda").bfloat16()
    calls = []
    real_up, real_fused = ops.upsample_bilinear, ops.conv_upcat_bias_act
    monkeypatch.setattr(ops, "upsample_bilinear", lambda *a, **kw: (calls.append("two"), real_up(*a, **kw))[1])
    monkeypatch.setattr(ops, "conv_upcat_bias_act", lambda *a, **kw: (calls.append("fused"), real_fused(*a, **kw))[1])
    with torch.no_grad():
        monkeypatch.setenv("GDKVM_UPCAT_FUSED", "1")
        model.segment(frames)
        assert calls == ["fused", "fused"]
        monkeypatch.setenv("GDKVM_UPCAT_FUSED", "0")
        model.segment(frames)
        assert calls == ["fused", "fused", "two", "two"]


def test_refusals_on_the_device(hip):
    """What the CPU test cannot reach: with a device present, shapes the band logic does not take are refused by the library (no launch),
    and the wrapper's own checks hold."""
    g = torch.Generator(device="cuda").manual_seed(3)
    lo, x2 = _rand(g, 1, 64, 7, 7), _rand(g, 1, 64, 14, 14)
    wt = _rand(g, 64, 128, 3, 3)
    b = torch.zeros(64, device="cuda")
    with pytest.raises(hip.GdkvmError):                     # not exactly 2x
        hip.conv_upcat_bias_act(lo, _rand(g, 1, 64, 15, 14), wt, b)
    with pytest.raises(hip.GdkvmError):                     # rows wider than 64 pixels
        hip.conv_upcat_bias_act(_rand(g, 1, 64, 2, 33), _rand(g, 1, 64, 4, 66), wt, b)
    with pytest.raises(hip.GdkvmError):                     # chunks of 64 channels
        hip.conv_upcat_bias_act(_rand(g, 1, 56, 7, 7), x2, _rand(g, 64, 120, 3, 3), b)
    assert hip.conv_upcat_bias_act(lo[:0], x2[:0], wt, b).shape == (0, 64, 14, 14)
