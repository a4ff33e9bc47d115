"""The three weight-gradient kernels of training are persistent: a workgroup (in conv3x3_wgrad_kernel: each of its two wave halves)
walks a stream of tiles or row slabs, reuses its LDS buffers, keeps the accumulators in registers and writes ONE fp32 partial block; a
second kernel adds the partial blocks in a fixed order.  A loop-carried mistake faults nothing: it multiplies stale or half-landed
operands, or drops a tile.  The older tests stay at zero or one tile per stream, so here

  * every frame carries values of its own and a stream walks three or four tiles (or a second one at the boundary), the reduce
    kernels run their unrolled-by-8 loops with and without tails, and both LDS-fit shrink loops of the plan are entered;
  * pure-Python mirrors of the host-side plans (wgrad_plan, stem_wgrad_grid, cw_splits) are pinned to the library through the
    *_workspace_bytes entry points, and every case asserts from its mirror that it reaches the regime it is here for: if somebody
    changes a grid, the case fails with a message instead of going back to one tile per workgroup unnoticed;
  * results are checked against fp64 sums over the same bf16 operands at the neighbouring tests' bounds, and the reference alone
    shows that those bounds see one lost tile a hundred times over."""
import pytest
import torch
import torch.nn.functional as F

from tests.test_conv_prefetch_gpu import _guarded_flat

pytestmark = pytest.mark.gpu

CL = dict(memory_format=torch.channels_last)
REVISIT = "the kernel's plan has changed: the shapes of this file must be worked out again"


# ---- mirrors of the host-side plans -----------------------------------------------------------------------------------------------------

def plan_conv3x3(n, c, h, w, k):
    """conv3x3_wgrad.hip's wgrad_plan: frames per tile, rows per tile, row tiles per frame, tiles, grid, and which LDS-fit loop ran."""
    assert c % 64 == 0 and k % 64 == 0 and 1 <= w <= 64 and h >= 1 and n >= 1
    maxpix, slots = 224, 9
    if h * w <= maxpix:
        th, fpt, tiles_y = h, min(maxpix // (h * w), n), 1
    else:
        fpt, th = 1, maxpix // w
        tiles_y = -(-h // th)
    fpt0, th0 = fpt, th

    def pieces():
        band_px, tpix = fpt * (th + 2) * (w + 2), fpt * th * w
        return (band_px * slots + 63) // 64, ((tpix + 31) // 32 * 32 * slots + 63) // 64

    def fits():
        return sum(pieces()) * 1024 <= 78 * 1024

    while not fits() and fpt > 1:
        fpt -= 1
    while not fits() and th > 1:
        th -= 1
        tiles_y = -(-h // th)
    assert fits()
    ntiles = -(-n // fpt) * tiles_y
    gy = (c // 64) * (k // 64)
    gx = min(max(256 // gy, 1), (ntiles + 1) // 2)
    return dict(fpt=fpt, th=th, tiles_y=tiles_y, ntiles=ntiles, gx=gx, gy=gy, fpt0=fpt0, th0=th0, pieces=pieces(),
                shrunk="frames" if fpt < fpt0 else "rows" if th < th0 else None)


def stream_counts(ntiles, streams):
    """Tiles walked by each of `streams` loops `for (t = s; t < ntiles; t += streams)`."""
    return [len(range(s, ntiles, streams)) for s in range(streams)]


def reduce_slices(gx):
    """(trips of the unrolled-by-8 loop, tail length) of each of the 8 slices of a reduce kernel over gx partial blocks."""
    per = (gx + 7) // 8
    counts = [max(0, min(gx, (s + 1) * per) - s * per) for s in range(8)]
    return per, [(m // 8, m % 8) for m in counts]


def plan_stem(n, h, w):
    """stem_conv_pool.hip's stem_wgrad_grid: tiles of 4 x 56 outputs of the [h/2, w/2] map on at most 768 workgroups."""
    tiles_x, tiles_y = -(-(w // 2) // 56), -(-(h // 2) // 4)
    ntiles = n * tiles_x * tiles_y
    return dict(tiles_x=tiles_x, tiles_y=tiles_y, ntiles=ntiles, gx=min(ntiles, 768))


def plan_strided(n, c, k, h, w, r, stride, pad):
    """gemm.hip's cw_splits and the rows of a split (whole 32-row slabs); `last`: the rows left to the last split."""
    ho, wo = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - r) // stride + 1
    m = n * ho * wo
    tiles = -(-k // 128) * (r * r * c // 64)
    splits = max(1, min(-(-1024 // tiles), -(-m // 256)))
    rows = (-(-m // splits) + 31) // 32 * 32
    return dict(m=m, ho=ho, wo=wo, splits=splits, rows=rows, last=m - (splits - 1) * rows, wide=k % 128 == 0)


# ---- the fp64 reference -----------------------------------------------------------------------------------------------------------------

def _tn(a, b):
    """a^T b of fp64 [M, K] and [M, C], as 32 batched products and their sum (one long, thin product is a single workgroup's work in a
    BLAS that does not split the inner dimension)."""
    m = a.shape[0]
    g = 32 if m >= 1024 else 1
    m0 = m // g * g
    out = torch.bmm(a[:m0].view(g, m0 // g, -1).transpose(1, 2), b[:m0].view(g, m0 // g, -1)).sum(0)
    return out + a[m0:].t() @ b[m0:] if m0 < m else out


def ref_wgrad(x, dy, r, stride, pad):
    """fp64 dW[k, c, u, v] = sum over (n, y, x) of dy[n, k, y, x] * xpad[n, c, stride y + u, stride x + v]: one product over the pixels
    per tap, on strided views of the padded input -- the weight gradient of conv2d(x, w, stride, pad) without a convolution library."""
    k, ho, wo = dy.shape[1:]
    c = x.shape[1]
    xp = F.pad(x.permute(0, 2, 3, 1).double(), (0, 0, pad, pad, pad, pad))
    d2 = dy.permute(0, 2, 3, 1).double().reshape(-1, k)
    out = torch.empty(k, c, r, r, dtype=torch.float64, device=x.device)
    for u in range(r):
        for v in range(r):
            xs = xp[:, u:u + stride * (ho - 1) + 1:stride, v:v + stride * (wo - 1) + 1:stride, :]
            out[:, :, u, v] = _tn(d2, xs.reshape(-1, c))
    return out


def lost_tile_gap(x, dy, ref, r, stride, pad, frames, rows, cols):
    """max |ref - the fp64 gradient with dy zeroed on frames x rows x cols (one tile's pixels)|."""
    cut = dy.clone()
    cut[frames[0]:frames[1], :, rows[0]:rows[1], cols[0]:cols[1]] = 0
    assert not torch.equal(cut, dy)
    return (ref_wgrad(x, cut, r, stride, pad) - ref).abs().max().item()


def _randn_bf16(shape, gen, **fmt):
    return torch.randn(*shape, device="cuda", generator=gen).bfloat16().contiguous(**fmt)


# ---- conv3x3_wgrad ------------------------------------------------------------------------------------------------------------------------

# (N, C, K, H, W) -> what the mirror must report: tiles, workgroups, tiles per wave-half stream (lowest, highest), and the case's own reason
WG_CASES = {
    (390, 256, 256, 7, 7): dict(ntiles=98, gx=16, streams=(3, 4), fpt=4, th=7, tiles_y=1, shrunk=None, last_frames=2, per=2),
    (410, 128, 128, 14, 14): dict(ntiles=410, gx=64, streams=(3, 4), fpt=1, th=14, tiles_y=1, shrunk=None, per=8, slices=[(1, 0)] * 8),
    (400, 64, 64, 28, 28): dict(ntiles=1600, gx=256, streams=(3, 4), fpt=1, th=8, tiles_y=4, shrunk=None, per=32, slices=[(4, 0)] * 8),
    (135, 192, 64, 28, 28): dict(ntiles=540, gx=85, streams=(3, 4), fpt=1, th=8, tiles_y=4, shrunk=None, per=11,
                                 slices=[(1, 3)] * 7 + [(1, 0)]),
    (130, 128, 128, 9, 56): dict(ntiles=390, gx=64, streams=(3, 4), fpt=1, th=3, tiles_y=3, shrunk="rows", th0=4),
    (2110, 256, 256, 2, 3): dict(ntiles=101, gx=16, streams=(3, 4), fpt=21, th=2, tiles_y=1, shrunk="frames", fpt0=37, last_frames=10),
    (129, 128, 128, 14, 14): dict(ntiles=129, gx=64, streams=(1, 2), fpt=1, th=14, tiles_y=1, shrunk=None),
}
C_ABI_CASE = (410, 128, 128, 14, 14)


def _wg_plan_checked(hip, case):
    """The mirror's plan of a case, pinned to the library's workspace size and to the case's table entry."""
    n, c, k, h, w = case
    want, p = WG_CASES[case], plan_conv3x3(n, c, h, w, k)
    got = int(hip.load().gdkvm_conv3x3_wgrad_workspace_bytes(n, c, h, w, k))
    assert got == p["gx"] * p["gy"] * 64 * 9 * 64 * 4, f"{case}: the library plans {got} bytes, the mirror {p}: {REVISIT}"
    counts = stream_counts(p["ntiles"], 2 * p["gx"])
    per, slices = reduce_slices(p["gx"])
    print(f"{case}: ntiles {p['ntiles']} gx {p['gx']} gy {p['gy']} frames/tile {p['fpt']} (from {p['fpt0']}) rows/tile {p['th']} "
          f"(from {p['th0']}) row tiles {p['tiles_y']} LDS pieces {p['pieces']} tiles per stream {min(counts)}-{max(counts)} "
          f"reduce per {per} slices {slices}")
    for key in ("ntiles", "gx", "fpt", "th", "tiles_y", "shrunk", "fpt0", "th0"):
        if key in want:
            assert p[key] == want[key], f"{case}: {key} = {p[key]}, expected {want[key]}: {REVISIT}"
    assert (min(counts), max(counts)) == want["streams"], f"{case}: tiles per stream {min(counts)}-{max(counts)}: {REVISIT}"
    if want["streams"] == (1, 2):                          # ntiles = 2 gx + 1: ONE stream (an even wave half) runs a second tile
        assert counts.count(2) == 1 and counts[0] == 2 and counts[1] == 1, f"{case}: {counts}: {REVISIT}"
    if "last_frames" in want:
        assert n - (n - 1) // p["fpt"] * p["fpt"] == want["last_frames"], f"{case}: ragged frame group: {REVISIT}"
    if "per" in want:
        assert per == want["per"], f"{case}: reduce per = {per}: {REVISIT}"
    if "slices" in want:
        assert slices == want["slices"], f"{case}: reduce (unrolled trips, tail) per slice = {slices}: {REVISIT}"
    return p


def test_plan_mirrors_agree_with_the_library(hip):
    """The three mirrors against the *_workspace_bytes entry points (which launch nothing) on every shape of this file and on the
    older tests' shapes, whose regime the module docstring states: at most one tile per stream there."""
    lib = hip.load()
    old = [(6, 64, 64, 28, 28), (3, 128, 128, 14, 14), (9, 256, 256, 7, 7), (2, 384, 128, 14, 14), (2, 192, 64, 28, 28),
           (3, 64, 192, 9, 13), (1, 128, 64, 64, 64), (5, 64, 64, 3, 2)]
    for case in list(WG_CASES) + old + [(77, 64, 64, 1, 1), (300, 64, 128, 55, 55), (1, 64, 64, 40, 64)]:
        n, c, k, h, w = case
        p = plan_conv3x3(n, c, h, w, k)
        assert int(lib.gdkvm_conv3x3_wgrad_workspace_bytes(n, c, h, w, k)) == p["gx"] * p["gy"] * 64 * 9 * 64 * 4, (case, p)
        if case in old:
            assert max(stream_counts(p["ntiles"], 2 * p["gx"])) == 1 and p["shrunk"] is None and reduce_slices(p["gx"])[0] < 8, (case, p)
    for n, c, h, w in STEM_CASES + [(3, 3, 112, 112), (2, 1, 64, 48), (1, 4, 130, 118), (9, 3, 20, 256)]:
        assert int(lib.gdkvm_stem_wgrad_workspace_bytes(n, h, w)) == plan_stem(n, h, w)["gx"] * 64 * 256 * 4, (n, c, h, w)
    for case in STRIDED_CASES + [(2, 64, 64, 12, 10, 3, 1, 1), (3, 128, 40, 9, 9, 1, 2, 0), (1, 64, 72, 16, 16, 5, 2, 2), (3, 64, 128, 28, 28, 3, 2, 1)]:
        n, c, k, h, w, r, stride, pad = case
        assert int(lib.gdkvm_conv_wgrad_strided_workspace_bytes(n, c, h, w, k, r, r, stride, pad)) == \
            plan_strided(*case)["splits"] * k * r * r * c * 4, case


_wg_cache = {}


def _wg_inputs(case):
    """(x, dy, fp64 reference) of a case: computed once and left unchanged.  The case that two tests share stays; of the others one is
    resident at a time (up to 80 MB of operands each)."""
    if case not in _wg_cache:
        for other in [o for o in _wg_cache if o != C_ABI_CASE]:
            del _wg_cache[other]
        n, c, k, h, w = case
        gen = torch.Generator(device="cuda").manual_seed(sum(case))
        x, dy = _randn_bf16((n, c, h, w), gen, **CL), _randn_bf16((n, k, h, w), gen, **CL)
        _wg_cache[case] = (x, dy, ref_wgrad(x, dy, 3, 1, 1))
    return _wg_cache[case]


@pytest.mark.parametrize("case", list(WG_CASES), ids=lambda c: "x".join(map(str, c)))
def test_conv3x3_wgrad_over_several_tiles_per_stream(hip, case):
    """gdkvm_conv3x3_wgrad where a wave half walks three or four tiles (at the boundary: a second one) == the fp64 sums over the same
    bf16 operands at test_convolution_weight_gradient's bound; the bound sees one lost tile a hundred times over; the same bits on a
    second call and in the channels_last order; and the sum of per-chunk calls in which no stream has a second tile meets the bound too."""
    n, c, k, h, w = case
    p = _wg_plan_checked(hip, case)
    x, dy, ref = _wg_inputs(case)
    npix = n * h * w
    bound = 1e-5 * npix ** 0.5 * max(1.0, ref.abs().max().item() / npix ** 0.5)

    # the reference alone: the second tile of stream 0 (the first one that a broken loop carry would lose)
    tile = 2 * p["gx"]
    assert tile < p["ntiles"], REVISIT
    fg, ty = divmod(tile, p["tiles_y"])
    frames, rows = (fg * p["fpt"], min(n, (fg + 1) * p["fpt"])), (ty * p["th"], min(h, (ty + 1) * p["th"]))
    gap = lost_tile_gap(x, dy, ref, 3, 1, 1, frames, rows, (0, w))
    print(f"{case}: tile {tile} (frames {frames}, rows {rows}) lost: max difference {gap:.3e} = {gap / bound:.0f} bounds")
    assert gap >= 100 * bound, f"{case}: a lost tile moves the gradient by {gap:.3e}, under 100 x the bound {bound:.3e}: choose other inputs"

    dw = hip.conv3x3_wgrad(x, dy)
    assert dw.dtype == torch.float32 and dw.shape == ref.shape and dw.is_contiguous()
    err = (dw.double() - ref).abs().max().item()

    # the same batch in chunks whose streams walk at most one tile each: no loop carry
    def carries(frames_):
        q = plan_conv3x3(frames_, c, h, w, k)
        return max(stream_counts(q["ntiles"], 2 * q["gx"])) > 1

    step = n
    while carries(step):
        step = (step + 1) // 2
    chunks = [(a, min(n, a + step)) for a in range(0, n, step)]
    assert len(chunks) >= 2, REVISIT
    total = torch.zeros_like(ref)
    for a, b in chunks:
        total += hip.conv3x3_wgrad(x[a:b], dy[a:b]).double()
    err_chunks = (total - ref).abs().max().item()
    print(f"{case}: max |dw - fp64| = {err:.3e} ({err / bound:.3f} bounds), in {len(chunks)} chunks of {step} frames {err_chunks:.3e} "
          f"({err_chunks / bound:.3f} bounds), bound {bound:.3e}")
    verdict = {(True, True): "both within", (False, True): "the WHOLE-BATCH call (several tiles per stream) left the bound, the per-chunk calls did not",
               (True, False): "the PER-CHUNK calls (one tile per stream) left the bound, the whole-batch call did not",
               (False, False): "the whole-batch call AND the per-chunk calls left the bound"}[(err <= bound, err_chunks <= bound)]
    assert err <= bound and err_chunks <= bound, f"{case}: {verdict}: {err:.3e} / {err_chunks:.3e} against {bound:.3e}"

    assert torch.equal(dw, hip.conv3x3_wgrad(x, dy)), f"{case}: a second call gives other bits"
    dwc = hip.conv3x3_wgrad(x, dy, channels_last=True)
    assert dwc.is_contiguous(**CL) and torch.equal(dwc, dw), f"{case}: the channels_last form gives other numbers"


def test_conv3x3_wgrad_c_abi_in_guarded_storage(hip):
    """gdkvm_conv3x3_wgrad with x, dy, the workspace (exactly the reported size, NaN-filled) and dw each in the middle of a NaN-filled
    buffer: the reduce kernel reads only partial blocks this call wrote (a finite result, the bits of ops.conv3x3_wgrad), every
    partial block is written, and no store lands outside the gx * gy blocks or outside dw."""
    case = C_ABI_CASE
    n, c, k, h, w = case
    p = _wg_plan_checked(hip, case)
    x, dy, _ = _wg_inputs(case)
    lib = hip.load()
    guard = 4096
    assert guard % 8 == 0 and guard >= w * max(c, k) + 8
    _, xv = _guarded_flat(x, guard)
    _, yv = _guarded_flat(dy, guard)
    need = int(lib.gdkvm_conv3x3_wgrad_workspace_bytes(n, c, h, w, k))
    assert need == p["gx"] * p["gy"] * 64 * 9 * 64 * 4
    wbuf, wv = _guarded_flat(torch.full((need // 4,), float("nan"), device="cuda"), guard)
    dbuf, dv = _guarded_flat(torch.full((k, c, 3, 3), float("nan"), device="cuda"), guard)
    assert all(t.data_ptr() % 16 == 0 for t in (xv, yv, wv, dv)) and wbuf.isnan().all() and dbuf.isnan().all()
    rc = lib.gdkvm_conv3x3_wgrad(xv.data_ptr(), yv.data_ptr(), dv.data_ptr(), wv.data_ptr(), need, n, c, h, w, k, hip.BF16,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.isfinite(dv).all(), "the result has non-finite elements: a partial block was read that this call did not write"
    assert torch.isfinite(wv).all(), "a partial block of the workspace was not (wholly) written"
    for name, buf, m in (("workspace", wbuf, wv.numel()), ("dw", dbuf, dv.numel())):
        assert buf[:guard].isnan().all() and buf[guard + m:].isnan().all(), f"a store landed outside the {name}"
    assert torch.equal(dv.view(k, c, 3, 3), hip.conv3x3_wgrad(x, dy))


# ---- stem_wgrad -----------------------------------------------------------------------------------------------------------------------------

# (N, C, H, W).  16 x 16 frames: an 8 x 8 map, two row tiles of 4 x 8 -> 2400 tiles on 768 workgroups; 36 x 120: an 18 x 60 map, 5 x 2
# tiles with the last row tile (2 rows) and the second column tile (4 columns) ragged -> 2500 tiles.  Three or four tiles a workgroup.
STEM_CASES = [(1200, 3, 16, 16), (1200, 1, 16, 16), (250, 4, 36, 120)]
STEM_PLANS = {(1200, 3, 16, 16): (1, 2, 2400), (1200, 1, 16, 16): (1, 2, 2400), (250, 4, 36, 120): (2, 5, 2500)}


@pytest.mark.parametrize("case", STEM_CASES, ids=lambda c: "x".join(map(str, c)))
def test_stem_wgrad_over_several_tiles_per_workgroup(hip, case):
    """ops.stem_wgrad (gdkvm_stem_wgrad_nchw) where a workgroup walks three or four tiles == the fp64 weight gradient of conv2d(x, w,
    stride 2, padding 3) on the bf16 operands at test_training_stem_convolution_on_the_stem_kernel's bound; the bound sees a lost
    tile; the same bits on a second call and in a channels_last parameter's layout."""
    n, c, h, w = case
    p = plan_stem(n, h, w)
    got = int(hip.load().gdkvm_stem_wgrad_workspace_bytes(n, h, w))
    assert got == p["gx"] * 64 * 256 * 4, f"{case}: the library plans {got} bytes, the mirror {p}: {REVISIT}"
    counts = stream_counts(p["ntiles"], p["gx"])
    print(f"{case}: tiles {p['tiles_x']} x {p['tiles_y']} per frame, {p['ntiles']} on {p['gx']} workgroups, {min(counts)}-{max(counts)} each")
    assert (p["tiles_x"], p["tiles_y"], p["ntiles"]) == STEM_PLANS[case] and p["gx"] == 768, f"{case}: {p}: {REVISIT}"
    assert (min(counts), max(counts)) == (3, 4), f"{case}: tiles per workgroup {min(counts)}-{max(counts)}: {REVISIT}"

    gen = torch.Generator(device="cuda").manual_seed(sum(case))
    x, dy = _randn_bf16((n, c, h, w), gen), _randn_bf16((n, 64, h // 2, w // 2), gen, **CL)
    ref = ref_wgrad(x, dy, 7, 2, 3)
    bound = 2e-5 * max(1.0, ref.abs().max().item()) * max(1.0, (n * h * w / 4) ** 0.5 / 64)

    # the reference alone: the first whole tile among the second tiles of the workgroups
    tile = next(t for t in range(p["gx"], p["ntiles"]) if t % p["tiles_x"] == 0 and t // p["tiles_x"] % p["tiles_y"] < max(1, p["tiles_y"] - 1))
    tx, t2 = tile % p["tiles_x"], tile // p["tiles_x"]
    ty, f = t2 % p["tiles_y"], t2 // p["tiles_y"]
    rows, cols = (4 * ty, min(h // 2, 4 * ty + 4)), (56 * tx, min(w // 2, 56 * tx + 56))
    gap = lost_tile_gap(x, dy, ref, 7, 2, 3, (f, f + 1), rows, cols)
    print(f"{case}: tile {tile} (frame {f}, rows {rows}, columns {cols}) lost: max difference {gap:.3e} = {gap / bound:.0f} bounds")
    assert gap >= 100 * bound, f"{case}: a lost tile moves the gradient by {gap:.3e}, under 100 x the bound {bound:.3e}: choose other inputs"

    dw = hip.stem_wgrad(x, dy)
    assert dw.dtype == torch.float32 and dw.shape == ref.shape and dw.is_contiguous()
    err = (dw.double() - ref).abs().max().item()
    print(f"{case}: max |dw - fp64| = {err:.3e} ({err / bound:.3f} bounds), bound {bound:.3e}")
    assert err <= bound
    assert torch.equal(dw, hip.stem_wgrad(x, dy)), f"{case}: a second call gives other bits"
    like = torch.empty(64, c, 7, 7, device="cuda").contiguous(**CL)
    dwc = hip.stem_wgrad(x, dy, like=like)
    assert dwc.stride() == like.stride() and torch.equal(dwc, dw), f"{case}: the channels_last form gives other numbers"


# ---- conv_wgrad_strided ---------------------------------------------------------------------------------------------------------------------

# (N, C, K, H, W, R, stride, pad) -> (rows M, splits, rows per split, rows of the last split, the 128-column form)
STRIDED_PLANS = {
    (9, 64, 64, 28, 28, 3, 2, 1): (1764, 7, 256, 228, False),       # split boundaries inside frames (196 rows each)
    (9, 64, 128, 28, 28, 3, 2, 1): (1764, 7, 256, 228, True),
    (209, 64, 128, 13, 13, 1, 2, 0): (10241, 41, 256, 1, True),     # 40 x 256 + 1: the last split holds a single row
    (209, 64, 72, 13, 13, 1, 2, 0): (10241, 41, 256, 1, False),     # and the 64-column form's second column tile has 8 of 64 columns
    (12, 64, 40, 20, 22, 5, 2, 2): (1320, 6, 224, 200, False),      # a 5 x 5 window, rows per split no multiple of 64
}
STRIDED_CASES = list(STRIDED_PLANS)


@pytest.mark.parametrize("case", STRIDED_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_wgrad_strided_over_several_row_splits(hip, case):
    """ops.conv_wgrad_strided (gdkvm_conv_wgrad_strided) with six or more row splits, a ragged last one, in the 64- and the 128-column
    form == the fp64 sums at test_strided_block_convolutions_forward_and_backward's bound, in both memory formats of the parameter,
    the same bits on a second call."""
    n, c, k, h, w, r, stride, pad = case
    p = plan_strided(*case)
    got = int(hip.load().gdkvm_conv_wgrad_strided_workspace_bytes(n, c, h, w, k, r, r, stride, pad))
    assert got == p["splits"] * k * r * r * c * 4, f"{case}: the library plans {got} bytes, the mirror {p}: {REVISIT}"
    print(f"{case}: M {p['m']} in {p['splits']} splits of {p['rows']} rows, the last {p['last']}; {'128' if p['wide'] else '64'}-column form")
    assert (p["m"], p["splits"], p["rows"], p["last"], p["wide"]) == STRIDED_PLANS[case], f"{case}: {p}: {REVISIT}"
    assert p["splits"] >= 6 and 0 < p["last"] < p["rows"], f"{case}: {p}: {REVISIT}"
    if p["m"] == 10241:
        assert p["last"] == 1, f"{case}: {p}: {REVISIT}"

    gen = torch.Generator(device="cuda").manual_seed(sum(case))
    x, dy = _randn_bf16((n, c, h, w), gen, **CL), _randn_bf16((n, k, p["ho"], p["wo"]), gen, **CL)
    ref = ref_wgrad(x, dy, r, stride, pad)
    bound = 2e-5 * max(1.0, ref.abs().max().item()) * max(1.0, p["m"] ** 0.5 / 64)
    first = None
    for like in (torch.empty(k, c, r, r, device="cuda"), torch.empty(k, c, r, r, device="cuda").contiguous(**CL)):
        dw = hip.conv_wgrad_strided(x, dy, like, stride, pad)
        assert dw.dtype == torch.float32 and dw.shape == ref.shape and dw.stride() == like.stride()
        err = (dw.double() - ref).abs().max().item()
        print(f"{case}: strides {tuple(like.stride())}: max |dw - fp64| = {err:.3e} ({err / bound:.3f} bounds), bound {bound:.3e}")
        assert err <= bound
        assert torch.equal(dw, hip.conv_wgrad_strided(x, dy, like, stride, pad)), f"{case}: a second call gives other bits"
        first = dw if first is None else first
        assert torch.equal(dw, first), f"{case}: the two memory formats give other numbers"


# ---- the training convolution above its grid size ---------------------------------------------------------------------------------------

def test_training_convolution_with_more_tiles_than_workgroups(hip):
    """ops.conv3x3 at (600, 64, 192, 9, 13): 600 frames are more tiles than the persistent forward kernel has workgroups, in the forward
    and in the 192 -> 64 data gradient (the same kernel on the flipped, transposed weights), where
    test_training_convolution_forward_and_data_gradient stays below; its bounds, against conv2d autograd in fp64 on the bf16-rounded
    operands.  With the weights packed ahead (the form a training step runs) the bits are the same."""
    n, c, k, h, w = 600, 64, 192, 9, 13
    gen = torch.Generator(device="cuda").manual_seed(n + c + k + h + w)
    x = _randn_bf16((n, c, h, w), gen, **CL).requires_grad_(True)
    wt = torch.nn.Parameter(torch.randn(k, c, 3, 3, device="cuda", generator=gen) / (9 * c) ** 0.5)      # fp32 master weights
    dy = _randn_bf16((n, k, h, w), gen)
    assert hip.conv3x3_train_served(x, wt, (1, 1), (1, 1), (1, 1), 1)
    y = hip.conv3x3(x, wt)
    dx, dw = torch.autograd.grad(y, (x, wt), dy)
    x64 = x.detach().double().requires_grad_(True)
    w64 = wt.detach().bfloat16().double().requires_grad_(True)
    y64 = F.conv2d(x64, w64, None, 1, 1)
    dx64, dw64 = torch.autograd.grad(y64, (x64, w64), dy.double())
    tol = 2.0 ** -7
    for name, a, b, f in (("y", y, y64, 1), ("dx", dx, dx64, 1), ("dw", dw, dw64, 2)):
        err, bound = (a.double() - b).abs().max().item(), f * tol * max(1.0, b.abs().max().item())
        print(f"{name}: max |got - fp64| = {err:.3e} ({err / bound:.3f} bounds), bound {bound:.3e}")
        assert a.dtype == (torch.float32 if name == "dw" else torch.bfloat16) and err <= bound, name
    with hip.train_packs([wt]):
        assert hip._train_packs_of(wt) is not None
        y1 = hip.conv3x3(x, wt)
        dx1, dw1 = torch.autograd.grad(y1, (x, wt), dy)
    assert torch.equal(y, y1) and torch.equal(dx, dx1) and torch.equal(dw, dw1)
