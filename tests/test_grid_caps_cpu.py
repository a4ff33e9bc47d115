"""tests/grid_caps.py against the kernel sources, and the shapes of tests/test_grid_caps_gpu.py against tests/grid_caps.py: (a) every cap
constant equals the one in the .hip file, so a changed cap fails here until the table follows; (b) every GPU case crosses the cap / trip
count / kernel arm it is there for; (c) the kernels' float-reciprocal divisions are exact for the shapes the GPU cases use."""
import os
import re

import numpy as np
import pytest

from tests import grid_caps as gc


@pytest.mark.parametrize("name", sorted(gc.CONSTANTS))
def test_constant_equals_the_source(name):
    assert gc.source_constant(name) == gc.CONSTANTS[name][0] == getattr(gc, name)


@pytest.mark.parametrize("name", sorted(gc.CONSTANTS))
def test_a_changed_constant_is_noticed(name, tmp_path):
    """The reader reads the number itself: from a copy of the source with the literals of this constant raised by one it returns another value."""
    value, fname, where, rx = gc.CONSTANTS[name]
    with open(os.path.join(gc.CSRC, fname)) as f:
        text = f.read()
    scope = text if where is None else gc.function_body(text, where)
    m = re.search(rx, scope)
    bumped = re.sub(r"\d+", lambda d: str(int(d.group()) + 1), m.group(1))
    if r"\1" in rx:                                             # a cap written twice (`if (blocks > cap) blocks = cap`): both places
        edited = scope[:m.start()] + m.group(0).replace(m.group(1), bumped) + scope[m.end():]
    else:
        edited = scope[:m.start(1)] + bumped + scope[m.end(1):]
    assert text.count(scope) == 1
    (tmp_path / fname).write_text(text.replace(scope, edited))
    assert gc.source_constant(name, str(tmp_path)) != value


# ------------------------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("dtype,shape", gc.BIAS_ACT_CASES)
def test_bias_act_cases(dtype, shape):
    g = gc.bias_act(shape, dtype)
    if shape[0] * shape[2] * shape[3] < 1000:                        # the small case: one workgroup, channels not kept
        assert not g.capped and g.blocks == 1 and not g.fixed and g.tail and not g.unrolled
        return
    assert g.capped and g.blocks == 2048 and g.nvec > 3 * 2048 * 256 and g.unrolled and g.tail and g.trips >= 2
    assert g.fixed == (shape[1] in (64,))                            # C / V = 8 or 16 divides the stride, C / V = 3 does not
    assert g.fixed or (2048 * 256) % (shape[1] // gc.vec(dtype)) == 2


@pytest.mark.parametrize("dtype,shape", gc.MAXPOOL_CASES)
def test_maxpool_cases(dtype, shape):
    g = gc.maxpool(shape, dtype)
    for k in (g.fused, g.fwd):
        assert k.capped and k.blocks == 4096 and k.total > 1048576 and k.trips == 2
    assert g.bwd.capped and g.bwd.trips >= 4


def test_stem_s2d_cases():
    (d0, s0, cp0), (d1, s1, cp1), (d2, s2, cp2) = gc.STEM_CASES
    g = gc.stem_s2d(s0, cp0, d0)
    assert g.capped and g.blocks == 8192 and g.total == 2134512 and g.trips == 2 and g.fast_path
    assert gc.vec(d1) == 8 and not gc.stem_s2d(s1, cp1, d1).fast_path          # bf16 on the general path
    assert gc.vec(d2) == 4 and not gc.stem_s2d(s2, cp2, d2).fast_path


def test_head_cases():
    (d0, s0, n0), (d1, s1, n1), (d2, s2, n2) = gc.HEAD_CASES
    for d, s in ((d0, s0), (d1, s1)):
        g = gc.head(s, d)
        assert g.logits.capped and g.logits.blocks == 4096 and g.logits.trips == 2
        assert g.bwd.capped and g.bwd.partial_rows == 512 and g.bwd.trips >= 8
    assert (gc.head(s0, d0).npix, gc.head(s1, d1).npix) == (132440, 67760)
    g = gc.head(s2, d2)
    assert g.bwd.capped and g.bwd.partial_rows == 512 and g.bwd.trips == 2 and not g.logits.capped and n2 == gc.HB_MAXC == s2[1] // gc.vec(d2)


def test_seg_loss_case():
    ni, c, h, w, hh, ww = gc.LOSS_CASE
    g = gc.seg_loss(ni, hh, ww)
    assert g.total == 527067 and g.capped and g.blocks == 2048 and g.trips == 2 and g.finalize_trips == 8
    assert not (hh == 4 * h and ww == 4 * w)                         # (the backward's general footprint loop)


@pytest.mark.parametrize("dtype,shape", gc.BN_CASES)
def test_bn_act_cases(dtype, shape):
    g = gc.bn_act(shape, dtype)
    for p in (g.fwd, g.bwd):
        assert p.red.capped and p.map.capped and p.nred <= 512 and p.nmap <= 2048
        assert p.red.steps >= 2 and p.map.steps >= 2                 # several walks per workgroup in both passes
        assert p.red.unrolled_trips >= 1 and p.red.tail_trips >= 1 and p.map.unrolled_trips >= 1 and p.map.tail_trips >= 1
        assert p.sum_trips >= 2 and p.nred * p.rpb_red >= shape[0] * shape[2] * shape[3] > (p.nred - 1) * p.rpb_red
    assert g.bwd.red.unrolled_trips >= 2
    assert g.fwd.active_lanes == (255 if shape[1] == 24 else 256)


def test_bn_relu_pool_cases():
    two, gather, refused = gc.BN_POOL_2X2, gc.BN_POOL_GATHER, gc.BN_POOL_REFUSED
    g = gc.bn_relu_pool(two)
    assert g.served and g.form == "2x2" and g.bwd_red.total == 536256 and g.bwd_red.capped and g.bwd_red.blocks == 512 and g.bwd_red.trips >= 2
    assert g.bwd_dx.capped and g.bwd_dx.blocks == 2048 and g.bwd_dx.trips == 2 and g.stats.red.capped and not g.pool_fwd.capped
    g = gc.bn_relu_pool(gather)
    assert g.served and g.form == "gather" and g.pixels == 4194048 and g.pixels + 256 == gc.BN_POOL_PIXEL_LIMIT
    assert g.bwd.red.capped and g.bwd.map.capped and g.bwd.red.unrolled_trips >= 2 and g.bwd.active_lanes == 255
    g = gc.bn_relu_pool(refused)
    assert not g.served and g.pixels >= gc.BN_POOL_PIXEL_LIMIT and refused[1] % 8 == 0


def test_upsample_cat_cases():
    wide, wide2x, rows, split, big = gc.UP_WIDE, gc.UP_WIDE_2X, gc.UP_ROWS, gc.UP_SPLIT, gc.UP_BWD_16X
    g, b = gc.upsample_cat(wide), gc.upsample_cat_bwd(wide)
    assert g.kernel == "row" and g.interp_trips == 2 and g.copy_tail and wide[6] * wide[1] // 8 == 528 and wide[6] * wide[4] // 8 == 528
    assert b.trips == 1 and wide[3] * wide[1] // 8 == 256 and not b.exact2x            # the backward's one-trip control
    g, g0, b = gc.upsample_cat(wide2x), gc.upsample_cat(wide2x, row_pairs=False), gc.upsample_cat_bwd(wide2x)
    assert g.kernel == "2x" and g0.kernel == "row/2x" and g.interp_trips == g0.interp_trips == 2 and (wide2x[3] + 1) * wide2x[1] // 8 == 336
    assert g.copy_tail and b.trips == 2 and b.exact2x and wide2x[3] * wide2x[1] // 8 == 320
    g = gc.upsample_cat(rows)
    assert g.kernel == "row" and g.capped and g.blocks == 4096 and rows[0] * rows[5] == 4200 and g.rows_per_block == 2 and g.launches == 1
    g = gc.upsample_cat(split)
    assert g.kernel == "row" and g.launches == 2 and g.per_launch == 16131 and g.capped
    sl = gc.UP_SPLIT_SLICES                                          # frames of the first launch, across the boundary, of the second launch
    assert sl[0].stop < g.per_launch and sl[1].start < g.per_launch < sl[1].stop and g.per_launch < sl[2].start and sl[2].stop == split[0]
    b = gc.upsample_cat_bwd(big)
    assert not b.exact2x and min(b.enlargement) >= 15.5


# ------------------------------------------------------------------------------------------------------------------ (c)
def _qdiv(n, d):
    """(int)(((float)n + 0.5f) * inv) with inv = 1.0f / d, in float32 as the kernels evaluate it."""
    inv = np.float32(1.0) / np.float32(d)
    return ((n.astype(np.float32) + np.float32(0.5)) * inv).astype(np.int32)


@pytest.mark.parametrize("nhw", [gc.BN_POOL_GATHER[:1] + gc.BN_POOL_GATHER[2:], (85598, 7, 7)])
def test_pool_gather_pixel_split_is_exact(nhw):
    """bn.hip pool_gather: m -> (n, ih, iw) through two reciprocal divisions, for every pixel index below N H W < 2^22."""
    n, h, w = nhw
    assert n * h * w < gc.BN_POOL_PIXEL_LIMIT
    m = np.arange(n * h * w, dtype=np.int32)
    img = _qdiv(m, h * w)
    assert np.array_equal(img, m // (h * w))
    r = m - img * (h * w)
    assert np.array_equal(_qdiv(r, w), r // w)


def test_upsample_row_split_is_exact():
    """upsample_cat's qdiv(row, 1 / H) at H = 65 for every row below 2^20, and the per-row column splits of the GPU gc."""
    hh = gc.UP_SPLIT[5]
    assert hh == 65
    rows = np.arange(gc.UPSAMPLE_ROW_LIMIT, dtype=np.int32)
    assert np.array_equal(_qdiv(rows, hh), rows // hh)
    for case in (gc.UP_WIDE, gc.UP_WIDE_2X, gc.UP_ROWS, gc.UP_SPLIT):
        n, c1, hl, wl, c2, H, W = case
        for cn in (c1 // 8, c2 // 8):                                # inv = 8.0f / C: the same float as 1.0f / (C / 8) for these C
            assert np.float32(8.0) / np.float32(cn * 8) == np.float32(1.0) / np.float32(cn)
            j = np.arange(max(W, wl + 1) * cn, dtype=np.int32)
            assert np.array_equal(_qdiv(j, cn), j // cn)
