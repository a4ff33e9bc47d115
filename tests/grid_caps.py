"""The host launch arithmetic of the streaming kernels (csrc/epilogue.hip, bn.hip, gates.hip head, loss.hip), restated in plain Python:
how many workgroups an entry point launches for a shape, whether that count hit its cap, and how many trips a thread / workgroup then
takes through its loops.  tests/test_grid_caps_cpu.py pins every constant below to the .hip source and proves that each shape of
tests/test_grid_caps_gpu.py crosses what it claims to cross; nothing here needs torch or a GPU."""
import os
import re
from types import SimpleNamespace as NS

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gdkvm_amd", "csrc")

# name -> (value, file, where, regex with ONE group holding the constant's expression).  `where` is the function whose body is searched
# (an extern "C" entry point, or the named helper / kernel), or None for a file-scope constexpr.
CONSTANTS = {
    "BIAS_ACT_CAP": (2048, "epilogue.hip", "gdkvm_bias_act", r"if \(blocks > ([^)]+)\) blocks = \1;"),
    "BIAS_ACT_UNR": (4, "epilogue.hip", "bias_act_kernel", r"constexpr int UNR = (\d+);"),
    "BIAS_RELU_MAXPOOL_CAP": (4096, "epilogue.hip", "gdkvm_bias_relu_maxpool", r"if \(blocks > ([^)]+)\) blocks = \1;"),
    "MAXPOOL_FWD_CAP": (4096, "epilogue.hip", "gdkvm_maxpool_fwd", r"if \(blocks > ([^)]+)\) blocks = \1;"),
    "MAXPOOL_BWD_CAP": (4096, "epilogue.hip", "gdkvm_maxpool_bwd", r"if \(blocks > ([^)]+)\) blocks = \1;"),
    "STEM_S2D_CAP": (8192, "epilogue.hip", "gdkvm_stem_s2d", r"if \(blocks > ([^)]+)\) blocks = \1;"),
    "UPSAMPLE_CAP_2X": (4096, "epilogue.hip", "gdkvm_upsample_cat", r"\(hl \+ 1\);\s*if \(blocks > ([^)]+)\) blocks = \1;"),
    "UPSAMPLE_CAP_ROW": (4096, "epilogue.hip", "gdkvm_upsample_cat", r"nn \* H;\s*if \(blocks > ([^)]+)\) blocks = \1;"),
    "UPSAMPLE_ROW_LIMIT": (1 << 20, "epilogue.hip", "gdkvm_upsample_cat", r"const int per = \(int\)\(\(\(([^)]+)\) - 1\) / \(unsigned\)H\);"),
    "UPSAMPLE_MAXV": (2, "epilogue.hip", "upsample_cat_bf16_kernel", r"constexpr int MAXV = (\d+);"),
    "UPSAMPLE_BWD_CAP": (4096, "epilogue.hip", "gdkvm_upsample_cat_bwd", r"if \(blocks > ([^)]+)\) blocks = \1;"),
    "HEAD_LOGITS_CAP": (4096, "gates.hip", "gdkvm_head_logits", r"if \(blocks > ([^)]+)\) blocks = \1;"),
    "HEAD_BWD_CAP": (512, "gates.hip", "gdkvm_head_bwd", r"if \(blocks > ([^)]+)\) blocks = \1;"),
    "HB_MAXC": (8, "gates.hip", None, r"constexpr int HB_MAXC = (\d+);"),
    "LOSS_MAX_PART": (2048, "loss.hip", None, r"constexpr int LOSS_MAX_PART = (\d+);"),
    "BN_MAX_PART": (512, "bn.hip", None, r"constexpr int BN_MAX_PART = (\d+);"),
    "BN_MAP_CAP": (2048, "bn.hip", "bn_plan", r"split\(([^,]+), \d+, p\.nmap, p\.rpb_map\);"),
    "BN_MAP_UNR": (4, "bn.hip", "bn_plan", r"split\([^,]+, (\d+), p\.nmap, p\.rpb_map\);"),
    "BN_FWD_RED_UNR": (8, "bn.hip", "gdkvm_bn_fwd_train", r"bn_plan\(rows, C, V, (\d+)\);"),
    "BN_BWD_RED_UNR": (4, "bn.hip", "gdkvm_bn_bwd", r"bn_plan\(rows, C, V, (\d+)\);"),
    "BN_POOL_FWD_RED_UNR": (8, "bn.hip", "gdkvm_bn_pool_fwd_train", r"bn_plan\(M, C, 8, (\d+)\);"),
    "BN_POOL_BWD_RED_UNR": (4, "bn.hip", "gdkvm_bn_pool_bwd", r"bn_plan\(M, C, 8, (\d+)\);"),
    "BN_POOL_DX_CAP": (2048, "bn.hip", "gdkvm_bn_pool_bwd", r"blocks < (\d+) \? blocks : \1\)"),
    "BN_POOL_FWD_CAP": (65536, "bn.hip", "gdkvm_bn_pool_fwd_train", r"blocks > (\d+) \? \1 : blocks"),
    "BN_POOL_PIXEL_LIMIT": (1 << 22, "bn.hip", "bn_pool_check", r"\(long long\)N \* H \* W >= \(([^)]+)\)"),
    "BN_SUM_ROWS_PER_TRIP": (128, "bn.hip", "sum_partials", r"b0 < nblk; b0 \+= ([^)]+)\)"),
}
globals().update({k: v[0] for k, v in CONSTANTS.items()})


def function_body(text, name):
    """The text between the braces of the first DEFINITION of `name` (a call or a declaration ends in ';' or ',' before any '{')."""
    for m in re.finditer(r"\b%s\s*\(" % re.escape(name), text):
        depth, i = 0, m.end() - 1
        while True:                                          # the matching ')' of the parameter list
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
            if depth == 0:
                break
        rest = text[i:].lstrip()
        if not rest.startswith("{"):
            continue
        start = i + text[i:].index("{")
        depth, j = 0, start
        while True:
            depth += {"{": 1, "}": -1}.get(text[j], 0)
            j += 1
            if depth == 0:
                return text[start:j]
    raise LookupError(name)


def source_constant(name, csrc=CSRC, table=None):
    """The value the .hip source gives the constant `name` of `table` (this file's CONSTANTS unless given; products and shifts of integer
    literals are evaluated)."""
    _, fname, where, rx = (CONSTANTS if table is None else table)[name]
    with open(os.path.join(csrc, fname)) as f:
        text = f.read()
    scope = text if where is None else function_body(text, where)
    found = re.findall(rx, scope)
    if len(found) != 1:
        raise LookupError(f"{name}: {len(found)} matches of {rx!r} in {fname}:{where}")
    expr = re.sub(r"(?<=\d)(ull|ll|u)\b", "", found[0])
    if not re.fullmatch(r"[\d\s*<()]+", expr):
        raise LookupError(f"{name}: {found[0]!r} is no product / shift of integer literals")
    return int(eval(expr, {"__builtins__": {}}))


def vec(dtype):
    """Elements per 16-byte access: 8 in bf16, 4 in fp32 (`dtype` a name or a torch dtype)."""
    s = str(dtype)
    if s.endswith("bfloat16") or s == "bf16":
        return 8
    if s.endswith("float32") or s == "fp32":
        return 4
    raise ValueError(dtype)


def _cdiv(a, b):
    return -(-a // b)


def pooled(n):
    return (n - 1) // 2 + 1


def grid_stride(total, cap, per_block=256):
    """min(ceil(total / per_block), cap) workgroups that stride over `total` items: the most trips any thread takes."""
    want = _cdiv(total, per_block)
    blocks = min(want, cap)
    return NS(total=total, blocks=blocks, capped=want > cap, trips=_cdiv(total, blocks * per_block))


def bias_act(shape, dtype):
    """gdkvm_bias_act on [N, C, H, W]: a thread owns T = ceil((nvec - i0) / stride) vectors, T // UNR unrolled trips and T % UNR tail trips."""
    n, c, h, w = shape
    v = vec(dtype)
    nvec = n * h * w * c // v
    g = grid_stride(nvec, BIAS_ACT_CAP)
    stride = g.blocks * 256
    t_max = _cdiv(nvec, stride)
    owned = {t_max} | ({t_max - 1} if nvec % stride else set())        # threads past nvec % stride own one vector fewer
    g.nvec, g.fixed = nvec, stride % (c // v) == 0
    g.unrolled = any(t // BIAS_ACT_UNR for t in owned)
    g.tail = any(t % BIAS_ACT_UNR for t in owned)
    return g


def maxpool(shape, dtype):
    """gdkvm_bias_relu_maxpool / gdkvm_maxpool_fwd (items: pooled pixel x channel group) and gdkvm_maxpool_bwd (input pixel x group)."""
    n, c, h, w = shape
    cg = c // vec(dtype)
    return NS(fused=grid_stride(n * pooled(h) * pooled(w) * cg, BIAS_RELU_MAXPOOL_CAP),
              fwd=grid_stride(n * pooled(h) * pooled(w) * cg, MAXPOOL_FWD_CAP),
              bwd=grid_stride(n * h * w * cg, MAXPOOL_BWD_CAP))


def stem_s2d(shape, cp, dtype):
    n, c, h, w = shape
    g = grid_stride(n * (h // 2) * (w // 2), STEM_S2D_CAP)
    g.fast_path = vec(dtype) == 8 and cp == 16 and c <= 4             # the bf16 stem case; everything else is the general path
    return g


def head(shape, dtype):
    """gdkvm_head_logits and gdkvm_head_bwd on [N, C, H, W]: a wave instruction covers ppw = 64 / G pixels, a workgroup 4 ppw."""
    n, c, h, w = shape
    per_block = 4 * (64 // (c // vec(dtype)))
    npix = n * h * w
    bwd = grid_stride(npix, HEAD_BWD_CAP, per_block)
    bwd.partial_rows = bwd.blocks
    return NS(npix=npix, logits=grid_stride(npix, HEAD_LOGITS_CAP, per_block), bwd=bwd)


def seg_loss(ni, h_out, w_out):
    g = grid_stride(ni * h_out * w_out, LOSS_MAX_PART)
    g.finalize_trips = _cdiv(g.blocks, 256)                           # partial rows per thread of the one finalize workgroup
    return g


def bn(rows, c, dtype, unr_red):
    """bn_plan(M, C, V, unr_red): nred x rpb_red for the reduction pass, nmap x rpb_map for the map pass; a workgroup walks its rows RP at
    a time, so it takes rpb / RP steps: steps // unr unrolled trips and steps % unr tail trips."""
    v = vec(dtype)
    g = c // v
    rp = 256 // g

    def split(cap, unr):
        trip = rp * unr
        want = _cdiv(rows, trip)
        blocks = max(1, min(want, cap))
        r = _cdiv(_cdiv(rows, blocks), rp) * rp
        steps = r // rp
        return NS(blocks=_cdiv(rows, r), rpb=r, capped=want > cap, steps=steps, unrolled_trips=steps // unr, tail_trips=steps % unr)

    red, mp = split(BN_MAX_PART, unr_red), split(BN_MAP_CAP, BN_MAP_UNR)
    return NS(G=g, RP=rp, active_lanes=rp * g, nred=red.blocks, rpb_red=red.rpb, nmap=mp.blocks, rpb_map=mp.rpb, red=red, map=mp,
              sum_trips=_cdiv(red.blocks, BN_SUM_ROWS_PER_TRIP))


def bn_act(shape, dtype):
    n, c, h, w = shape
    return NS(fwd=bn(n * h * w, c, dtype, BN_FWD_RED_UNR), bwd=bn(n * h * w, c, dtype, BN_BWD_RED_UNR))


def bn_relu_pool(shape):
    """gdkvm_bn_pool_fwd_train / gdkvm_bn_pool_bwd on bf16 [N, C, H, W]: refused at 2^22 pixels; backward on 2 x 2 pixel blocks where the
    channel groups divide 256, as a per-pixel gather inside the plain BatchNorm passes otherwise."""
    n, c, h, w = shape
    m, g = n * h * w, c // 8
    out = NS(pixels=m, served=m < BN_POOL_PIXEL_LIMIT and c % 8 == 0 and g <= 256, form="2x2" if 256 % g == 0 else "gather")
    if not out.served:
        return out
    out.stats = bn(m, c, "bf16", BN_POOL_FWD_RED_UNR)
    out.pool_fwd = grid_stride(n * pooled(h) * pooled(w) * g, BN_POOL_FWD_CAP)
    if out.form == "2x2":
        items = n * ((h + 1) // 2) * ((w + 1) // 2) * g
        out.bwd_red, out.bwd_dx = grid_stride(items, BN_MAX_PART), grid_stride(items, BN_POOL_DX_CAP)
    else:
        out.bwd = bn(m, c, "bf16", BN_POOL_BWD_RED_UNR)
    return out


def upsample_cat(case, row_pairs=True):
    """gdkvm_upsample_cat for (n, c1, hl, wl, c2, H, W): launches over image ranges below 2^20 rows, the kernel each takes, its workgroups
    and the trips of its inner loops (interpolated vectors, copy vectors past the first MAXV * 256)."""
    n, c1, hl, wl, c2, hh, ww = case
    c1n, c2n = c1 // 8, c2 // 8
    per = (UPSAMPLE_ROW_LIMIT - 1) // hh
    exact2x = hh == 2 * hl and ww == 2 * wl
    nn = min(n, per)
    if exact2x and row_pairs:
        kernel, g, interp = "2x", grid_stride(nn * (hl + 1), UPSAMPLE_CAP_2X, 1), _cdiv((wl + 1) * c1n, 256)
    elif exact2x:
        kernel, g, interp = "row/2x", grid_stride(nn * hh, UPSAMPLE_CAP_ROW, 1), _cdiv((wl + 1) * c1n, 256)
    else:
        kernel, g, interp = "row", grid_stride(nn * hh, UPSAMPLE_CAP_ROW, 1), _cdiv(ww * c1n, UPSAMPLE_MAXV * 256)
    return NS(launches=_cdiv(n, per), per_launch=per, kernel=kernel, blocks=g.blocks, capped=g.capped, rows_per_block=g.trips,
              interp_trips=interp, copy_tail=ww * c2n > UPSAMPLE_MAXV * 256)


def upsample_cat_bwd(case):
    n, c1, hl, wl, c2, hh, ww = case
    g = grid_stride(n * hl, UPSAMPLE_BWD_CAP, 1)
    return NS(blocks=g.blocks, capped=g.capped, rows_per_block=g.trips, trips=_cdiv(wl * (c1 // 8), 256),
              exact2x=hh == 2 * hl and ww == 2 * wl, enlargement=(hh / hl, ww / wl))


# ---------------------------------------------------------------------------------------------------------------------------------------
# The shapes tests/test_grid_caps_gpu.py runs ([N, C, H, W] unless stated; dtypes by name) -- here, so that tests/test_grid_caps_cpu.py can
# prove what each of them crosses without a GPU.
BIAS_ACT_CASES = [("bf16", (5, 64, 239, 241)), ("bf16", (13, 24, 243, 243)), ("fp32", (5, 64, 169, 171)), ("fp32", (13, 12, 243, 243)),
                  ("bf16", (2, 24, 5, 7))]
MAXPOOL_CASES = [("bf16", (9, 64, 255, 253)), ("fp32", (5, 64, 255, 253))]
STEM_CASES = [("bf16", (36, 3, 486, 488), 16), ("bf16", (2, 5, 20, 24), 24), ("fp32", (2, 5, 20, 24), 24)]
HEAD_CASES = [("bf16", (43, 64, 56, 55), 2), ("fp32", (22, 64, 56, 55), 4), ("bf16", (3, 64, 75, 73), 8)]          # (.., classes)
LOSS_CASE = (9, 3, 60, 61, 243, 241)                                                                              # (NI, C, h, w, H, W)
BN_CASES = [("bf16", (5, 64, 231, 229)), ("fp32", (3, 64, 211, 209)), ("bf16", (13, 24, 233, 231))]
BN_POOL_2X2, BN_POOL_GATHER, BN_POOL_REFUSED = (21, 64, 113, 111), (256, 24, 127, 129), (257, 8, 127, 129)
# (n, c1, hl, wl, c2, H, W)
UP_WIDE, UP_WIDE_2X, UP_ROWS, UP_SPLIT = (2, 128, 17, 16, 128, 35, 33), (2, 128, 9, 20, 128, 18, 40), (70, 8, 28, 3, 8, 60, 7), (16400, 8, 32, 2, 8, 65, 5)
UP_SPLIT_SLICES = (slice(0, 3), slice(16127, 16135), slice(16392, 16400))         # the second straddles the launch boundary at frame 16131
UP_BWD_16X = (1, 8, 3, 3, 8, 50, 47)
