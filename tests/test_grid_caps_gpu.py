"""The streaming kernels of csrc/epilogue.hip, bn.hip, gates.hip (head) and loss.hip PAST their grid caps and one-trip loops: every case
here launches the capped number of workgroups, or takes a second trip through an inner loop, or selects an arm (`fixed = false`, the bf16
general space-to-depth path, the gather backward next to its 2^22-pixel limit, the several-launch split) that the small shapes of
tests/test_kpff_argmax_gpu.py and tests/test_train_side_gpu.py never reach.  tests/test_grid_caps_cpu.py proves, from the launch arithmetic
restated in tests/grid_caps.py, that each shape crosses what it is here for.  References and bounds are those of the small-shape tests
(torch in fp32 / fp64 on the same operands, bit-equality where they assert bits), computed on the device.

Sums over all rows (BatchNorm dgamma / dbeta / running statistics, head dW / db) were first measured for torch's own fp32 computation
against the fp64 reference at these sizes (figures in the tests' docstrings): it stays an order of magnitude or more inside the small-shape
bounds, so those bounds are kept.  Each test prints torch's figure beside the kernel's."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import grid_caps as gc

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
CL = dict(memory_format=torch.channels_last)


def _ids(cases):
    return ["%s-%s" % (c[0], "x".join(map(str, c[1]))) for c in cases]


def _err(a, b):
    return (a.double() - b.double()).abs().max().item()


# ------------------------------------------------------------------------------------------------------------------ epilogue.hip
@pytest.mark.parametrize("dtype,shape", gc.BIAS_ACT_CASES, ids=_ids(gc.BIAS_ACT_CASES))
def test_bias_act_unrolled_body_and_moving_channels(hip, dtype, shape):
    """gdkvm_bias_act at 2048 workgroups x 4.4 vectors per thread (unrolled body, then tail), with C / V = 8 and 16 (the thread keeps its
    channels over every trip) and C / V = 3 (it does not; also on one uncapped workgroup): bit for bit the fp32 expression rounded once."""
    dt = DT[dtype]
    torch.manual_seed(sum(shape))
    x = torch.randn(shape, device="cuda").to(dt).contiguous(**CL)
    r = torch.randn(shape, device="cuda").to(dt).contiguous(**CL)
    b = torch.randn(shape[1], device="cuda")
    for res, relu in ((None, True), (r, True), (r, False), (None, False)):
        want = (x.float() if res is None else x.float() + res.float()) + b.reshape(1, -1, 1, 1)     # the kernel's order
        want = (want.clamp_min(0) if relu else want).to(dt)
        got = hip.bias_act_(x.clone(**CL), b, res, relu)
        assert torch.equal(got, want), (res is not None, relu, (got != want).sum().item())


@pytest.mark.parametrize("dtype,shape", gc.MAXPOOL_CASES, ids=_ids(gc.MAXPOOL_CASES))
def test_bias_relu_maxpool_past_its_cap(hip, dtype, shape):
    dt = DT[dtype]
    n, c, h, w = shape
    torch.manual_seed(sum(shape))
    x = torch.randn(shape, device="cuda").to(dt).contiguous(**CL)
    b = torch.randn(c, device="cuda")
    got = hip.bias_relu_maxpool(x, b)
    want = F.max_pool2d(F.relu(x.float() + b.reshape(1, -1, 1, 1)).to(dt).float(), 3, 2, 1).to(dt)
    assert got.shape == want.shape and got.is_contiguous(**CL)
    assert torch.equal(got, want)


@pytest.mark.parametrize("dtype,shape", gc.MAXPOOL_CASES, ids=_ids(gc.MAXPOOL_CASES))
def test_maxpool_forward_and_gather_backward_past_their_caps(hip, dtype, shape):
    """Two trips forward, five backward: values bit-equal to torch's max_pool2d, gradients equal to torch's backward, ties included."""
    dt = DT[dtype]
    torch.manual_seed(sum(shape))
    x = (torch.randn(shape, device="cuda") * 2).round().div(2).clamp_min(0).to(dt).contiguous(**CL)        # ReLU-like, many ties
    dy = torch.randn(shape[0], shape[1], gc.pooled(shape[2]), gc.pooled(shape[3]), device="cuda").to(dt).contiguous(**CL)
    xa, xb = x.clone(**CL).requires_grad_(True), x.clone(**CL).float().requires_grad_(True)
    ya = hip.maxpool3x3s2(xa)
    yb = F.max_pool2d(xb, 3, 2, 1)
    assert torch.equal(ya.float(), yb)
    ya.backward(dy); yb.backward(dy.float())
    err = _err(xa.grad, xb.grad)
    print("maxpool", dtype, shape, "dx err", err)
    assert err <= (2.0 ** -7 if dt == torch.bfloat16 else 1e-6) * max(1.0, xb.grad.abs().max().item())


@pytest.mark.parametrize("dtype,shape,cp", gc.STEM_CASES, ids=_ids(gc.STEM_CASES))
def test_stem_s2d_past_its_cap_and_on_the_general_path(hip, dtype, shape, cp):
    dt = DT[dtype]
    n, c, h, w = shape
    x = torch.randn(shape, generator=torch.Generator(device="cuda").manual_seed(sum(shape)), device="cuda").to(dt)
    xs = hip.stem_s2d(x, cp)
    want = torch.zeros(n, cp, h // 2, w // 2, dtype=dt, device="cuda")
    want[:, :4 * c] = F.pixel_unshuffle(x, 2)
    assert xs.is_contiguous(**CL) and torch.equal(xs, want)


# ------------------------------------------------------------------------------------------------------------------ gates.hip (head)
@pytest.mark.parametrize("dtype,shape,ncls", gc.HEAD_CASES, ids=_ids(gc.HEAD_CASES))
def test_head_past_both_caps(hip, dtype, shape, ncls):
    """ops.head against conv2d in fp64 with the small-shape test's bounds: the forward past 4096 workgroups, the backward on 512 partial rows
    (9 trips per wave; 2 trips at 8 classes); the same bits on a second run.
    torch's own fp32 conv2d backward against the same fp64 reference, relative to max(1, |reference|max), on an MI355X: dW 7.5e-7 .. 1.0e-6,
    db 2.2e-8 .. 1.9e-7 (the kernel: 1.3e-7 .. 2.7e-7 and 5.0e-8 .. 3.0e-7) -- the small-shape bound of 1e-5 holds with room and is kept."""
    dt = DT[dtype]
    n, c, hh, ww = shape
    torch.manual_seed(sum(shape) + ncls)
    x = torch.randn(shape, device="cuda").to(dt).contiguous(**CL).requires_grad_(True)
    conv = torch.nn.Conv2d(c, ncls, 1).cuda()
    gz = torch.randn(n, ncls, hh, ww, device="cuda").to(dt)
    z = hip.head(x, conv.weight, conv.bias)
    assert z.is_contiguous() and z.dtype == dt
    z.backward(gz)

    def reference(prec):
        xr = x.detach().to(prec).requires_grad_(True)
        wr, br = conv.weight.detach().to(prec).requires_grad_(True), conv.bias.detach().to(prec).requires_grad_(True)
        zr = F.conv2d(xr, wr, br)
        zr.backward(gz.to(prec))
        return zr.detach(), xr.grad, wr.grad, br.grad

    z64, dx64, dw64, db64 = reference(torch.float64)
    _, _, dw32, db32 = reference(torch.float32)
    wscale, bscale = max(1.0, dw64.abs().max().item()), max(1.0, db64.abs().max().item())
    print("head", dtype, shape, ncls, "dW err / scale: kernel %.3g torch fp32 %.3g; db: kernel %.3g torch fp32 %.3g (bound 1e-5)" % (
        _err(conv.weight.grad, dw64) / wscale, _err(dw32, dw64) / wscale, _err(conv.bias.grad, db64) / bscale, _err(db32, db64) / bscale))
    tol = 2.0 ** -7 if dt == torch.bfloat16 else 1e-5
    assert _err(z, z64) <= tol * max(1.0, z64.abs().max().item())
    assert _err(x.grad, dx64) <= tol * max(1.0, dx64.abs().max().item())
    assert conv.weight.grad.dtype == torch.float32 and _err(conv.weight.grad, dw64) <= 1e-5 * wscale
    assert _err(conv.bias.grad, db64) <= 1e-5 * bscale
    g1 = (x.grad.clone(), conv.weight.grad.clone(), conv.bias.grad.clone())
    x.grad = None; conv.zero_grad(set_to_none=True)
    hip.head(x, conv.weight, conv.bias).backward(gz)
    assert all(torch.equal(a, b) for a, b in zip(g1, (x.grad, conv.weight.grad, conv.bias.grad)))


# ------------------------------------------------------------------------------------------------------------------ loss.hip
@pytest.mark.parametrize("tdt", [torch.uint8, torch.int64], ids=["u8", "i64"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_fused_objective_on_2048_partial_rows(hip, dtype, tdt):
    """527 067 pixels: LOSS_MAX_PART workgroups take two trips and the finalize adds eight partial rows per thread; 30 % unlabelled.  Value
    and gradient against the fp64 restatement of test_fused_objective_ignores_unlabelled_pixels."""
    ni, c, h, w, H, W = gc.LOSS_CASE
    torch.manual_seed(sum(gc.LOSS_CASE))
    z = (2.0 * torch.randn(ni, c, h, w, device="cuda")).to(DT[dtype])
    tgt = torch.randint(0, c, (ni, H, W), device="cuda")
    tgt[torch.rand(ni, H, W, device="cuda") < 0.3] = 255
    za = z.clone().requires_grad_(True)
    loss = hip.seg_loss(za, tgt.to(tdt), 0.7, 1.0)
    loss.backward()
    zb = z.double().requires_grad_(True)
    up = F.interpolate(zb, size=(H, W), mode="bilinear", align_corners=False)
    ce = F.cross_entropy(up, tgt, ignore_index=255)
    p = up.softmax(1) * (tgt != 255).unsqueeze(1)
    oh = torch.stack([(tgt == k) for k in range(c)], 1).double()
    dice = 1.0 - ((2 * (p * oh).sum((0, 2, 3)) + 1.0) / (p.sum((0, 2, 3)) + oh.sum((0, 2, 3)) + 1.0)).mean()
    ref = ce + 0.7 * dice
    ref.backward()
    gerr = _err(za.grad, zb.grad) / zb.grad.abs().max().item()
    print("seg_loss", dtype, tdt, "loss", loss.item(), "ref", ref.item(), "grad err / scale", gerr)
    assert abs(loss.item() - ref.item()) <= 1e-5 * max(1.0, abs(ref.item()))
    assert gerr <= (2.0 ** -7 if dtype == "bf16" else 1e-4)


# ------------------------------------------------------------------------------------------------------------------ bn.hip
def _bn_reference(prec, x, w, b, res, relu, dy, mask, eps=1e-5):
    """F.batch_norm (+ residual) (+ the ReLU mask of the run under test) in `prec` on the device, with autograd and running statistics."""
    xr = x.detach().to(prec).requires_grad_(True)
    wr, br = w.detach().to(prec).requires_grad_(True), b.detach().to(prec).requires_grad_(True)
    rr = None if res is None else res.detach().to(prec).requires_grad_(True)
    rm, rv = torch.zeros(x.shape[1], dtype=prec, device=x.device), torch.ones(x.shape[1], dtype=prec, device=x.device)
    y = F.batch_norm(xr, rm, rv, wr, br, True, 0.1, eps)
    if rr is not None:
        y = y + rr
    if relu:
        y = y * mask.to(prec)
    y.backward(dy.to(prec))
    return y.detach(), xr.grad, wr.grad, br.grad, (None if rr is None else rr.grad), rm, rv


@pytest.mark.parametrize("mode", ["relu", "res_relu"])
@pytest.mark.parametrize("dtype,shape", gc.BN_CASES, ids=_ids(gc.BN_CASES))
def test_bn_act_on_capped_grids(hip, dtype, shape, mode):
    """gdkvm_bn_fwd_train / gdkvm_bn_bwd with 485 .. 487 partial rows (four trips of sum_partials), 17 row walks per reduction workgroup
    (unrolled trips and a tail) and 5 per map workgroup, also at G = 3 (255 active lanes): fp64 F.batch_norm autograd, the bounds of
    test_bn_act_forward_backward.  torch's own fp32 batch_norm against the same reference on an MI355X: running mean 3.5e-8 .. 5.2e-8
    (bound 1e-5), running variance 2.4e-7 .. 3.8e-7 (1e-4), dgamma 1.3e-7 .. 2.5e-7 and dbeta 6.8e-8 .. 1.9e-7 of max(1, |reference|max)
    (the kernel: 4.3e-8 .. 7.3e-8, 3.9e-7 .. 1.2e-6, 1.3e-7 .. 6.5e-7, 1.2e-7 .. 2.4e-7): the small-shape bounds hold with room and are kept.
    dgamma and dbeta are fp32 sums of fp32 products whatever the I/O type, so in bf16 they are also held to the fp32 case's 2e-4: one
    partial row dropped out of 487 moves such a sum by about 1 / sqrt(487) = 4.5e-2 of its scale, too close to the bf16 bound of 3e-2."""
    dt = DT[dtype]
    torch.manual_seed(sum(shape) + len(mode))
    has_res = "res" in mode
    x = (3.0 + 2.0 * torch.randn(shape, device="cuda")).to(dt).contiguous(**CL)
    res = torch.randn(shape, device="cuda").to(dt).contiguous(**CL) if has_res else None
    w = torch.rand(shape[1], device="cuda") + 0.5
    b = 0.3 * torch.randn(shape[1], device="cuda")
    dy = torch.randn(shape, device="cuda").to(dt).contiguous(**CL)
    rm, rv = torch.zeros(shape[1], device="cuda"), torch.ones(shape[1], device="cuda")
    xg = x.clone(**CL).requires_grad_(True)
    wg, bg = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    rg = None if res is None else res.clone(**CL).requires_grad_(True)
    y = hip.bn_act(xg, wg, bg, rm, rv, rg, 0.1, 1e-5, True)
    assert y.dtype == dt and y.is_contiguous(**CL)
    y.backward(dy)
    mask = y.detach() > 0
    y_ref, dx_ref, dw_ref, db_ref, dr_ref, rm_ref, rv_ref = _bn_reference(torch.float64, x, w, b, res, True, dy, mask)
    _, _, dw32, db32, _, rm32, rv32 = _bn_reference(torch.float32, x, w, b, res, True, dy, mask)
    wscale, bscale = max(dw_ref.abs().max().item(), 1.0), max(db_ref.abs().max().item(), 1.0)
    tol = 3e-2 if dt == torch.bfloat16 else 2e-4
    print("bn_act", dtype, shape, mode, "kernel / torch fp32: rm %.3g / %.3g (1e-5)  rv %.3g / %.3g (1e-4)  dgamma/scale %.3g / %.3g  dbeta/scale %.3g / %.3g (%g)" % (
        _err(rm, rm_ref), _err(rm32, rm_ref), _err(rv, rv_ref), _err(rv32, rv_ref), _err(wg.grad, dw_ref) / wscale, _err(dw32, dw_ref) / wscale,
        _err(bg.grad, db_ref) / bscale, _err(db32, db_ref) / bscale, tol))
    eps_io = 2.0 ** -8 if dt == torch.bfloat16 else 1e-5
    assert _err(y, y_ref) <= eps_io * max(1.0, y_ref.abs().max().item())
    assert _err(rm, rm_ref) <= 1e-5 and _err(rv, rv_ref) <= 1e-4
    assert _err(xg.grad, dx_ref) <= tol * max(dx_ref.abs().max().item(), 1e-6)
    assert _err(wg.grad, dw_ref) <= min(tol, 2e-4) * wscale
    assert _err(bg.grad, db_ref) <= min(tol, 2e-4) * bscale
    if has_res:
        assert _err(rg.grad, dr_ref) <= tol * max(dr_ref.abs().max().item(), 1.0)


def _bn_pool_both_ways(hip, shape):
    n, c, hh, ww = shape
    torch.manual_seed(sum(shape))
    x = (torch.randn(shape, device="cuda") * 4).round().div(4).bfloat16().contiguous(**CL)            # coarse values: ties in the windows
    g, b = torch.rand(c, device="cuda") + 0.5, torch.randn(c, device="cuda") * 0.2
    dy = torch.randn(n, c, gc.pooled(hh), gc.pooled(ww), device="cuda").bfloat16().contiguous(**CL)

    def run(fused):
        xa, ga, ba = x.clone(**CL).requires_grad_(True), g.clone().requires_grad_(True), b.clone().requires_grad_(True)
        rm, rv = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
        if fused:
            y = hip.bn_relu_pool(xa, ga, ba, rm, rv, 0.1, 1e-5)
        else:
            y = hip.maxpool3x3s2(hip.bn_act(xa, ga, ba, rm, rv, None, 0.1, 1e-5, True))
        y.backward(dy)
        return y.detach(), xa.grad, ga.grad, ba.grad, rm, rv

    assert hip.bn_relu_pool_served(x)
    return run(False), run(True)


@pytest.mark.parametrize("shape", [gc.BN_POOL_2X2, gc.BN_POOL_GATHER], ids=["2x2", "gather"])
def test_batchnorm_relu_maxpool_on_capped_grids(hip, shape):
    """ops.bn_relu_pool against ops.maxpool3x3s2(ops.bn_act(..)) under the rules of test_batchnorm_relu_maxpool_as_one_op.  2 x 2 form: 536 256
    items on 512 (sums) and 2048 (dx) workgroups.  Gather form: 4 194 048 pixels, 256 below the limit of its float-reciprocal pixel split,
    509 partial rows, 255 active lanes: bit for bit."""
    (ya, dxa, dga, dba, rma, rva), (yb, dxb, dgb, dbb, rmb, rvb) = _bn_pool_both_ways(hip, shape)
    assert torch.equal(ya, yb) and torch.equal(rma, rmb) and torch.equal(rva, rvb)          # forward: the same bits
    d = (dxa.float() - dxb.float()).abs()
    print("bn_relu_pool", shape, "dgamma diff / scale %.3g  dbeta %.3g  dx max diff %.3g, moved %.3g" % (
        _err(dga, dgb) / max(1.0, dga.abs().max().item()), _err(dba, dbb) / max(1.0, dba.abs().max().item()), d.max().item(), (d > 0).float().mean().item()))
    for a_, b_ in ((dga, dgb), (dba, dbb)):
        assert (a_ - b_).abs().max() <= 1e-5 * max(1.0, a_.abs().max().item())
    assert d.max() <= 2.0 ** -7 * max(1.0, dxa.float().abs().max().item()) and (d > 0).float().mean() <= 1e-2
    if 256 % (shape[1] // 8):
        assert torch.equal(dxa, dxb) and torch.equal(dga, dgb)                               # (the gather form: bit for bit)


def test_batchnorm_relu_maxpool_refuses_2_22_pixels(hip):
    """At 2^22 pixels and beyond the gather's reciprocal divisions are no longer exact: not served, and the call says so."""
    n, c, hh, ww = gc.BN_POOL_REFUSED
    x = torch.zeros(n, c, hh, ww, device="cuda", dtype=torch.bfloat16).contiguous(**CL)
    assert not hip.bn_relu_pool_served(x)
    with pytest.raises(hip.GdkvmError, match="2\\^22"):
        hip.bn_relu_pool(x, torch.ones(c, device="cuda"), torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda"), torch.ones(c, device="cuda"))


# ------------------------------------------------------------------------------------------------------------------ upsample_cat
def _lo_skip(case):
    n, c1, hl, wl, c2, H, W = case
    torch.manual_seed(sum(case))
    lo = torch.randn(n, c1, hl, wl, device="cuda").bfloat16().contiguous(**CL)
    sk = torch.randn(n, c2, H, W, device="cuda").bfloat16().contiguous(**CL)
    return lo, sk


@pytest.mark.parametrize("case", [gc.UP_WIDE, gc.UP_WIDE_2X, gc.UP_ROWS], ids=["wide", "wide2x", "rows"])
def test_upsample_cat_second_trips_and_row_cap(hip, case):
    """Rows of 528 interpolated and 528 copied vectors (a second trip of both loops), 336 column-pair vectors at exactly 2x on both kernels,
    and 4200 rows on 4096 workgroups: F.interpolate in fp32 with one bf16 rounding; the skip half bit for bit."""
    n, c1, hl, wl, c2, H, W = case
    lo, sk = _lo_skip(case)
    got = hip.upsample_cat(lo, sk)
    up = F.interpolate(lo.float(), size=(H, W), mode="bilinear", align_corners=False)
    assert got.shape == (n, c1 + c2, H, W) and got.is_contiguous(**CL)
    assert torch.equal(got[:, c1:], sk)
    assert (got[:, :c1].float() - up).abs().max() <= 2.0 ** -7 * up.abs().max()     # one bf16 rounding of an fp32 blend
    os.environ["GDKVM_UPSAMPLE_ROW_PAIRS"] = "0"                                    # the row-at-a-time kernel gives the same bits
    try:
        assert torch.equal(hip.upsample_cat(lo, sk), got)
        assert torch.equal(hip.upsample_bilinear(lo, (H, W)), got[:, :c1])
    finally:
        del os.environ["GDKVM_UPSAMPLE_ROW_PAIRS"]
    assert torch.equal(hip.upsample_bilinear(lo, (H, W)), got[:, :c1])


def test_upsample_cat_general_kernel_in_several_launches(hip):
    """16400 frames x 65 rows on the general kernel: two launches over image ranges (16131 frames fit below 2^20 rows), frame for frame
    the small-batch result either side of the boundary."""
    case = gc.UP_SPLIT
    n, c1, hl, wl, c2, H, W = case
    lo, sk = _lo_skip(case)
    got = hip.upsample_cat(lo, sk)
    for sl in gc.UP_SPLIT_SLICES:
        part = hip.upsample_cat(lo[sl].contiguous(**CL), sk[sl].contiguous(**CL))
        assert torch.equal(got[sl], part)
        up = F.interpolate(lo[sl].float(), size=(H, W), mode="bilinear", align_corners=False)
        assert (part[:, :c1].float() - up).abs().max() <= 2.0 ** -7 * up.abs().max()
    assert torch.equal(got[:, c1:], sk)


@pytest.mark.parametrize("case", [gc.UP_WIDE, gc.UP_WIDE_2X, gc.UP_ROWS, gc.UP_BWD_16X], ids=["wide", "wide2x", "rows", "16x"])
def test_upsample_cat_backward_second_trip_and_wide_window(hip, case):
    """gdkvm_upsample_cat_bwd with 256 (one trip, the control) and 320 (two trips) vectors per low-resolution row, on the general and the
    exactly-2x arm, and with a 16x enlargement in the candidate window: fp64 autograd, the bound of test_upsample_cat_backward."""
    n, c1, hl, wl, c2, H, W = case
    lo, sk = _lo_skip(case)
    lo.requires_grad_(True); sk.requires_grad_(True)
    dout = torch.randn(n, c1 + c2, H, W, device="cuda").bfloat16().contiguous(**CL)
    hip.upsample_cat(lo, sk).backward(dout)
    lo64 = lo.detach().double().requires_grad_(True)
    F.interpolate(lo64, size=(H, W), mode="bilinear", align_corners=False).backward(dout[:, :c1].double())
    assert torch.equal(sk.grad, dout[:, c1:])
    err = _err(lo.grad, lo64.grad)
    print("upsample_cat_bwd", case, "err", err, "scale", lo64.grad.abs().max().item())
    assert err <= 2.0 ** -7 * max(lo64.grad.abs().max().item(), 1.0)
