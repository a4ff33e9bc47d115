"""The bf16 (and fp32) kernels that multiply and accumulate, bit for bit against the ONE right answer on exactly summable inputs
(tests/exact_inputs.py): operands on dyadic grids, so every product and partial sum is an exact fp32 number whatever the order, and the
kernel's output must be the fp64 restatement (F.conv2d, @, max_pool2d in double, on the device) rounded once to nearest-even.  No
tolerance anywhere: every comparison is assert_bits against round_once.  A dropped tap, truncation, round-half-away, a rounding before the
residual or a bias through bf16 changes at least one bit of these cases (tests/test_exact_inputs_cpu.py).  The shapes are the smallest at
which each form still has its ragged tile, second chunk, second workgroup or wide row."""
import pytest
import torch

from tests import exact_inputs as X

pytestmark = pytest.mark.gpu

CL = dict(memory_format=torch.channels_last)
BF16, F32 = torch.bfloat16, torch.float32


def to(t, dtype=BF16):
    """An fp64 operand as the kernel takes it: cast (exact on these grids), feature maps and weights channels_last."""
    t = t.to(dtype)
    return t.contiguous(**CL) if t.dim() == 4 else t.contiguous()


def check(got, ref):
    X.assert_exactly_summable(ref)
    X.assert_bits(got, ref.exact())


def operands(make, case):
    return X.on(make(case), "cuda")


# ---- inference convolutions with their epilogue ----
@pytest.mark.parametrize("case", X.CONV_C64)
def test_conv_bias_act_64_channel_kernel(hip, case):
    """conv_bias_act kernel 4 (conv3x3_c64), plain and packed weights; ReLU on and off, with and without the residual."""
    o = operands(X.conv_operands, case)
    x, wt, b, r = to(o.x), to(o.w), to(o.b, F32), to(o.r)
    pk = hip.conv3x3_pack_weights(wt)
    for (relu, res), ref in X.conv_refs(o).items():
        for packed in (None, pk):
            check(hip.conv_bias_act(x, wt, b, r if res else None, 1, 1, relu, 4, packed), ref)


def test_the_comparison_sees_one_tap_and_a_bf16_bias_on_the_device(hip):
    """The check is not vacuous where it runs: the same kernel given a weight with ONE element (a 1/8) set to zero, or the bias rounded to
    bf16, no longer returns the right bits."""
    o = operands(X.conv_operands, X.CONV_C64[0])
    ref = X.conv_refs(o)[(False, True)]
    x, wt, b, r = to(o.x), to(o.w), to(o.b, F32), to(o.r)
    check(hip.conv_bias_act(x, wt, b, r, 1, 1, False, 4), ref)
    hit = o.w.clone()
    hit.view(-1)[int(torch.nonzero(o.w.reshape(-1).abs() == 1 / 8)[0])] = 0
    for wrong in (hip.conv_bias_act(x, to(hit), b, r, 1, 1, False, 4), hip.conv_bias_act(x, wt, b.bfloat16().float(), r, 1, 1, False, 4)):
        with pytest.raises(AssertionError, match="elements differ"):
            X.assert_bits(wrong, ref.exact())


@pytest.mark.parametrize("case", X.CONV_TILE)
def test_conv_bias_act_tile_kernel_and_its_variants(hip, case):
    """conv_bias_act kernel 5 (conv3x3_tile), the wave-grid variants 6, 7, 8, 11 (10 where K % 128 == 0) and kernel 0 (the choice by shape),
    each on plain and on packed weights."""
    o = operands(X.conv_operands, case)
    x, wt, b, r = to(o.x), to(o.w), to(o.b, F32), to(o.r)
    pk = hip.conv3x3_pack_weights(wt)
    kernels = (0, 5, 6, 7, 8, 11) + ((10,) if case[4] % 128 == 0 else ())
    for (relu, res), ref in X.conv_refs(o).items():
        for kernel in kernels:
            for packed in (None, pk):
                check(hip.conv_bias_act(x, wt, b, r if res else None, 1, 1, relu, kernel, packed), ref)


@pytest.mark.parametrize("case", X.CONV_IGEMM)
def test_conv_bias_act_implicit_gemm_kernel(hip, case):
    """conv_bias_act kernel 9 (conv_igemm): 5x5 / 3x3 / 1x1 windows, strides 1 and 2, rows wider than 64 pixels."""
    o = operands(X.conv_operands, case)
    x, wt, b, r = to(o.x), to(o.w), to(o.b, F32), to(o.r)
    pk = hip.conv_igemm_pack_weights(wt)
    for (relu, res), ref in X.conv_refs(o).items():
        check(hip.conv_bias_act(x, wt, b, r if res else None, o.stride, o.pad, relu, hip.CONV_KERNEL_IGEMM, pk), ref)


@pytest.mark.parametrize("case", X.CONV_DOWN)
def test_conv_down_bias_act_both_outputs(hip, case):
    """conv_down_bias_act: the block's first convolution (bias, ReLU on and off) and its 1x1 branch (bias given and None), one launch."""
    o = operands(X.down_operands, case)
    x, wt, wd, b, bd = to(o.x), to(o.w), to(o.wd), to(o.b, F32), to(o.bd, F32)
    pk, pkd = hip.conv_igemm_pack_weights(wt), hip.conv_igemm_pack_weights(wd)
    refs = X.down_refs(o)
    for relu in (True, False):
        for branch_bias in (True, False):
            y, yd = hip.conv_down_bias_act(x, wt, b, pk, wd, pkd, bd if branch_bias else None, o.stride, relu)
            check(y, refs[("y", relu)])
            check(yd, refs[("yd", branch_bias)])


@pytest.mark.parametrize("case", X.CONV_CAT)
def test_conv_cat_bias_act(hip, case):
    """conv_cat_bias_act: the convolution over [x1 ; x2] without the concatenated tensor, plain and packed weights."""
    o = operands(X.cat_operands, case)
    x1, x2, wt, b, r = to(o.x1), to(o.x2), to(o.w), to(o.b, F32), to(o.r)
    pk = hip.conv3x3_pack_weights(wt)
    for (relu, res), ref in X.cat_refs(o).items():
        for packed in (None, pk):
            check(hip.conv_cat_bias_act(x1, x2, wt, b, r if res else None, relu, 0, packed), ref)


@pytest.mark.parametrize("case", X.CONV_UPCAT)
def test_conv_upcat_bias_act_and_the_enlargement_alone(hip, case):
    """conv_upcat_bias_act against the exact 2x bilinear enlargement (align_corners = false) of lo, concatenated with x2 and convolved in
    fp64: lo holds multiples of 16, the enlarged values are integers and the kernel's bf16 rounding of them changes nothing.
    upsample_bilinear (2x) and upsample_cat (2x) alone give that same enlargement."""
    o = operands(X.upcat_operands, case)
    lo, x2, wt, b, r = to(o.lo), to(o.x2), to(o.w), to(o.b, F32), to(o.r)
    pk = hip.conv3x3_pack_weights(wt)
    refs = X.upcat_refs(o)
    up = refs.pop("up")
    check(hip.upsample_bilinear(lo, x2.shape[2:]), up)
    both = hip.upsample_cat(lo, x2)
    check(both[:, :lo.shape[1]], up)
    assert torch.equal(both[:, lo.shape[1]:], x2)
    for (relu, res), ref in refs.items():
        check(hip.conv_upcat_bias_act(lo, x2, wt, b, r if res else None, relu, pk), ref)


# ---- stem ----
@pytest.mark.parametrize("case", X.STEM)
def test_stem_conv_pool(hip, case):
    """stem_conv_pool == max_pool(relu(conv + bias)) rounded once (max commutes with the rounding)."""
    o = operands(X.stem_operands, case)
    check(hip.stem_conv_pool(to(o.xs), to(o.w), to(o.b, F32)), X.stem_refs(o)["y"])


@pytest.mark.parametrize("case", X.STEM_NCHW)
def test_stem_conv_pool_nchw(hip, case):
    o = operands(X.stem_nchw_operands, case)
    check(hip.stem_conv_pool_nchw(o.x.to(BF16).contiguous(), to(o.w), to(o.b, F32)), X.stem_nchw_refs(o)["y"])


# ---- training convolutions: forward and data gradient in bf16, the weight gradient in fp32 == the exact integer sum ----
@pytest.mark.parametrize("case", X.TRAIN_CONV)
def test_training_conv3x3_forward_and_both_gradients(hip, case):
    o = operands(X.train_conv_operands, case)
    refs = X.train_conv_refs(o)
    x, wt = to(o.x).requires_grad_(True), o.w.float().requires_grad_(True)              # fp32 master weights
    y = hip.conv3x3(x, wt)
    y.backward(to(o.dy))
    check(y.detach(), refs["y"])
    check(x.grad, refs["dx"])
    check(wt.grad, refs["dw"])


@pytest.mark.parametrize("case", X.TRAIN_WGRAD)
def test_conv3x3_wgrad_in_both_memory_orders(hip, case):
    o = operands(X.train_conv_operands, case)
    ref = X.train_conv_refs(o)["dw"]
    x, dy = to(o.x), to(o.dy)
    check(hip.conv3x3_wgrad(x, dy), ref)
    dwc = hip.conv3x3_wgrad(x, dy, channels_last=True)
    assert dwc.is_contiguous(**CL)
    check(dwc, ref)


@pytest.mark.parametrize("case", X.TRAIN_S2)
def test_conv_s2_block_forward_and_backward(hip, case):
    """ops.conv_s2_block: both outputs, dx over both branches in one sum, both weight gradients."""
    o = operands(X.train_s2_operands, case)
    refs = X.train_s2_refs(o)
    x = to(o.x).requires_grad_(True)
    w = torch.nn.Parameter(o.w.float().contiguous(**CL))
    wd = torch.nn.Parameter(o.wd.float())
    y, yd = hip.conv_s2_block(x, w, wd)
    dx, dw, dwd = torch.autograd.grad((y, yd), (x, w, wd), (to(o.gy), to(o.gyd)))
    for got, name in ((y.detach(), "y"), (yd.detach(), "yd"), (dx, "dx"), (dw, "dw"), (dwd, "dwd")):
        check(got, refs[name])


@pytest.mark.parametrize("case", X.WGRAD_STRIDED)
def test_conv_wgrad_strided(hip, case):
    o = operands(X.wgrad_strided_operands, case)
    ref = X.wgrad_strided_refs(o)["dw"]
    x, dy = to(o.x), to(o.dy)
    for like in (torch.empty(o.wshape, device="cuda"), torch.empty(o.wshape, device="cuda").contiguous(**CL)):
        dw = hip.conv_wgrad_strided(x, dy, like, o.stride, o.pad)
        assert dw.stride() == like.stride()
        check(dw, ref)


@pytest.mark.parametrize("case", X.TRAIN_STEM)
def test_training_stem_conv_and_its_weight_gradient(hip, case):
    o = operands(X.train_stem_operands, case)
    refs = X.train_stem_refs(o)
    x, w, gy = o.x.to(BF16).contiguous(), torch.nn.Parameter(o.w.float()), to(o.gy)
    y = hip.stem_conv(x, w)
    check(y.detach(), refs["y"])
    check(torch.autograd.grad(y, w, gy)[0], refs["dw"])
    check(hip.stem_wgrad(x, gy), refs["dw"])


# ---- token products and the head ----
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("case", X.GEMM)
def test_gemm_nt_and_the_token_major_weight_gradient(hip, case, dtype):
    """gemm_nt (C = a bt^T + bias) in `dtype`; wgrad (gemm_tn: a^T b2 in fp32), without and with the column sums from the same launch."""
    o = operands(X.gemm_operands, case)
    refs = X.gemm_refs(o)
    a, bt, b2 = to(o.a, dtype), to(o.bt, dtype), to(o.b2, dtype)
    check(hip.gemm_nt(a, bt, to(o.bias, F32)), refs[("c", dtype)])
    check(hip.wgrad(a, b2), refs["d"])
    d, cs = hip.wgrad(a, b2, colsum=True)
    check(d, refs["d"])
    check(cs, refs["colsum"])


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("case", X.TOKEN_LINEAR)
def test_token_linear_forward_and_backward(hip, case, dtype):
    """token_linear on 1001 rows, 64 -> 40: y and dx in `dtype`, dW and db in fp32.  The bias reaches the product's epilogue as fp32
    (ops._TokenLinear hands gemm_nt `bias.float()`; gemm.hip adds it to the fp32 accumulator), so the restatement does not round it."""
    o = operands(X.token_linear_operands, case)
    refs = X.token_linear_refs(o)
    x = to(o.x, dtype).requires_grad_(True)
    w, b = o.w.float().requires_grad_(True), o.b.float().requires_grad_(True)
    y = hip.token_linear(x, w, b)
    y.backward(to(o.dy, dtype))
    check(y.detach(), refs[("y", dtype)])
    check(x.grad, refs[("dx", dtype)])
    check(w.grad, refs["dw"])
    check(b.grad, refs["db"])


@pytest.mark.parametrize("case", X.PROJ_ROWS)
def test_proj_rows(hip, case):
    o = operands(X.proj_rows_operands, case)
    ref = X.proj_rows_refs(o)["out"]
    X.assert_exactly_summable(ref)
    want = ref.exact()
    outs = hip.proj_rows(to(o.x), hip.pack_rows_weight(o.w.float()), to(o.b, F32), o.widths)
    assert len(outs) == len(o.widths)
    c0 = 0
    for got, width in zip(outs, o.widths):
        X.assert_bits(got, want[:, c0:c0 + width])
        c0 += width


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("case", X.HEAD)
def test_head_logits(hip, case, dtype):
    n, c, h, w, ncls = case
    if dtype == F32 and ncls > c // 4 or dtype == BF16 and ncls > c // 8:
        pytest.skip("more classes than lanes per pixel")
    o = operands(X.head_operands, case)
    got = hip.head_logits(to(o.x, dtype), o.w.reshape(ncls, c).float().contiguous(), to(o.b, F32))
    assert got.is_contiguous()
    check(got, X.head_refs(o)[("z", dtype)])


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("case", X.HEAD_BWD)
def test_head_backward(hip, case, dtype):
    """ops.head: the logits, dx in `dtype`, dW and db in fp32 from the one-pass backward."""
    o = operands(X.head_operands, case)
    refs = X.head_refs(o)
    x = to(o.x, dtype).requires_grad_(True)
    w, b = torch.nn.Parameter(o.w.float()), torch.nn.Parameter(o.b.float())
    z = hip.head(x, w, b)
    z.backward(o.gz.to(dtype).contiguous())
    check(z.detach(), refs[("z", dtype)])
    check(x.grad, refs[("dx", dtype)])
    check(w.grad, refs["dw"])
    check(b.grad, refs["db"])


# ---- epilogue passes ----
@pytest.mark.parametrize("shape", X.BIAS_ACT)
def test_bias_act(hip, shape):
    o = operands(X.bias_act_operands, shape)
    b = to(o.b, F32)
    for (dtype, relu, res), ref in X.bias_act_refs(o).items():
        check(hip.bias_act_(to(o.x, dtype), b, to(o.r, dtype) if res else None, relu), ref)


@pytest.mark.parametrize("shape", X.POOL)
def test_bias_relu_maxpool(hip, shape):
    o = operands(X.pool_operands, shape)
    for dtype, ref in X.pool_refs(o).items():
        check(hip.bias_relu_maxpool(to(o.x, dtype), to(o.b, F32)), ref)
