"""conv3x3_tile's four-wave forms cut 14- and 7-wide maps into 112-pixel tiles that run ACROSS frame boundaries: a group of 4 (16) frames
is one stacked image of seven tiles, and two consecutive frames of a tile share ONE zero halo row in the LDS band.  What that can get wrong:
a halo row read from the neighbouring frame, a tile's rows attributed to the wrong frame or row, a ragged last group, a workgroup whose
second tile has another phase than its first.

The layer is called the way the model calls it (kernel 5, packed weights) on exactly summable inputs (tests/exact_inputs.py: integers and
eighths, every partial sum an exact fp32 number), and compared with torch.nn.functional.conv2d in fp32 on the same values, rounded once:
torch.equal, no tolerance.  Every frame carries its own offset, so a row that leaks through the shared zero row changes the sum."""
import pytest
import torch
import torch.nn.functional as F

from tests import exact_inputs as X

pytestmark = pytest.mark.gpu

CL = dict(memory_format=torch.channels_last)
KERNEL = 5                  # conv3x3_tile, wave grid by shape: the four-wave forms at these maps (K % 128 == 0: <4, 2>, else <2, 2>)


def _operands(n, c, h, w, k):
    """fp64 CPU operands: integers in [-8, 8] plus a per-frame offset (distinct for n <= 37), weights m / 8, fp32-only biases."""
    g = X.generator("stacked", n, c, h, w, k)
    offs = (torch.arange(n) % 37 - 18).double().view(n, 1, 1, 1)
    return X.integers(g, n, c, h, w) + offs, X.weights(g, k, c, 3, 3), X.biases(g, k), X.integers(g, n, k, h, w)


def _acc32(x, wt, check64=True):
    """conv2d in fp32 on the CPU; exact on these inputs in any order, which the fp64 convolution confirms."""
    acc = F.conv2d(x.float(), wt.float(), None, 1, 1)
    if check64:
        assert torch.equal(acc.double(), F.conv2d(x, wt, None, 1, 1)), "the fp32 reference is not exact"
    return acc


def _want(acc, b, r, relu):
    v = acc + b.float().view(1, -1, 1, 1)
    if r is not None:
        v = v + r.float()
    return (v.relu() if relu else v).bfloat16().contiguous(**CL)


def _dev(t, dtype=torch.bfloat16):
    t = t.to(dtype).cuda()
    return t.contiguous(**CL) if t.dim() == 4 else t.contiguous()


def _check_epilogues(hip, x, wt, b, r, acc, epilogues=((True, False), (True, True), (False, False), (False, True)), split=None):
    xd, wd, bd, rd = _dev(x), _dev(wt), _dev(b, torch.float32), _dev(r)
    pk = hip.conv3x3_pack_weights(wd)
    for relu, res in epilogues:
        if split is None:
            got = hip.conv_bias_act(xd, wd, bd, rd if res else None, 1, 1, relu, KERNEL, pk)
        else:
            x1, x2 = xd[:, :split].contiguous(**CL), xd[:, split:].contiguous(**CL)
            got = hip.conv_cat_bias_act(x1, x2, wd, bd, rd if res else None, relu, KERNEL, pk)
        X.assert_bits(got.cpu(), _want(acc, b, r if res else None, relu))


# 14 x 14, groups of 4 frames: a lone ragged group (1, 3), an exact group (4), a group and a remainder (5, 9); every phase 0 .. 6 from
# n = 4 on.  7 x 7, groups of 16: likewise (1, 2, 15 | 16 | 17, 33), with the tiles of four frame segments from n = 15 on.
@pytest.mark.parametrize("k", [32, 128])       # <2, 2> with 8-byte stores / <4, 2> with the permuted 16-byte epilogue
@pytest.mark.parametrize("hw,n", [(14, 1), (14, 3), (14, 4), (14, 5), (14, 9), (7, 1), (7, 2), (7, 15), (7, 16), (7, 17), (7, 33)])
def test_stacked_tiles_exact(hip, hw, n, k):
    """Residual on and off, ReLU on and off, bit for bit."""
    x, wt, b, r = _operands(n, 128, hw, hw, k)
    _check_epilogues(hip, x, wt, b, r, _acc32(x, wt))


def test_stacked_tiles_concatenated_input(hip):
    """conv_cat_bias_act (C1 = 64, C - C1 = 64): the second chunk comes from the second tensor, with its own pixel pitch."""
    x, wt, b, r = _operands(5, 128, 14, 14, 128)
    _check_epilogues(hip, x, wt, b, r, _acc32(x, wt), epilogues=((True, True), (False, False)), split=64)


def test_stacked_tiles_256_channels(hip):
    """7 x 7, C = K = 256, one exact group of 16 frames: four chunks per tile and two channel groups in the grid."""
    x, wt, b, r = _operands(16, 256, 7, 7, 256)
    _check_epilogues(hip, x, wt, b, r, _acc32(x, wt), epilogues=((True, True), (False, False)))


def test_second_tile_of_the_same_phase(hip):
    """300 frames of 14 x 14 at K = 32: 525 tiles on a grid of 511 (the largest multiple of 7 under 512), so fourteen workgroups take a
    second tile 511 further on -- of the same phase, with the band geometry they computed once."""
    x, wt, b, r = _operands(300, 128, 14, 14, 32)
    _check_epilogues(hip, x, wt, b, r, _acc32(x, wt, check64=False), epilogues=((True, True), (False, False)))


@pytest.mark.parametrize("case", [(2, 128, 28, 28, 128), (3, 128, 16, 10, 128), (3, 128, 16, 10, 32)])
def test_unstacked_maps_keep_their_tiling(hip, case):
    """A 28-wide map tiles 112 pixels exactly (rows of one frame) and 10 does not divide 112: both keep the row tiles, same bits."""
    x, wt, b, r = _operands(*case)
    _check_epilogues(hip, x, wt, b, r, _acc32(x, wt), epilogues=((True, True), (False, False)))


@pytest.mark.parametrize("hw,n", [(14, 9), (7, 33)])
def test_stacked_tiles_random_inputs(hip, hw, n):
    """Random inputs against the fp32 convolution of the same bf16 values, at the bound of the band-fetch tests (2^-7 of the largest
    value: one bf16 rounding of the output is 2^-9 of it)."""
    g = torch.Generator().manual_seed(1000 * hw + n)
    c = k = 128
    x = torch.randn(n, c, hw, hw, generator=g).bfloat16()
    wt = (torch.randn(k, c, 3, 3, generator=g) / (9 * c) ** 0.5).bfloat16()
    b = torch.randn(k, generator=g)
    r = torch.randn(n, k, hw, hw, generator=g).bfloat16()
    xd, wd, bd, rd = _dev(x), _dev(wt), _dev(b, torch.float32), _dev(r)
    got = hip.conv_bias_act(xd, wd, bd, rd, 1, 1, False, KERNEL, hip.conv3x3_pack_weights(wd)).cpu().float()
    want = F.conv2d(x.float(), wt.float(), b, 1, 1) + r.float()
    err = (got - want).abs().max().item()
    bound = 2.0 ** -7 * max(1.0, want.abs().max().item())
    print(f"max |got - want| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
