"""The host arithmetic of gdkvm_kpff_fwd_train, gdkvm_kpff_bwd_pre and gdkvm_proj_rows (csrc/kpff.hip), restated in plain Python: how a
grid is cut into tiles, which arm an (I/O type, channel counts, workspace) selects, which form of the bf16 arm a batch selects on a device
of `cus` compute units, how many trips a thread of kpff_bwd_pre_kernel takes, and where the projections change their tile.
tests/test_kpff_forms_cpu.py pins every constant below to the .hip source and proves that each case of
tests/test_kpff_train_forms_gpu.py selects what it claims to select; nothing here needs torch or a GPU."""
from types import SimpleNamespace as NS

from tests import grid_caps as gc

LDS_LIMIT = 160 * 1024

# name -> (value, file, where, regex with ONE group holding the constant's expression): the format of tests/grid_caps.py CONSTANTS.
CONSTANTS = {
    "KPFF_TM": (64, "kpff.hip", None, r"constexpr int KPFF_TM = (\d+);"),
    "KPFF_PAD16": (16, "kpff.hip", None, r"constexpr int KPFF_PAD16 = (\d+);"),
    "KPFF_OT": (1, "kpff.hip", None, r"constexpr int KPFF_OT = (\d+);"),
    "FULL_WIDTH_MAX": (16, "kpff.hip", "gdkvm_kpff_fwd_train", r"else if \(w <= (\d+)\) rows ="),
    "COL_TILE_ROWS": (4, "kpff.hip", "gdkvm_kpff_fwd_train", r"else \{ rows = (\d+); cols = \d+; \}"),
    "COL_TILE_COLS": (16, "kpff.hip", "gdkvm_kpff_fwd_train", r"else \{ rows = \d+; cols = (\d+); \}"),
    "LDS_LIMIT_TILE": (LDS_LIMIT, "kpff.hip", "gdkvm_kpff_fwd_train", r"if \(lds1 > ([^)]+)\)"),
    "LDS_LIMIT_PAIR": (LDS_LIMIT, "kpff.hip", "gdkvm_kpff_fwd_train", r"const bool pair = 2 \* lds1 <= ([^&]+?) &&"),
    "LDS_LIMIT_SPLIT": (LDS_LIMIT, "kpff.hip", "gdkvm_kpff_fwd_train", r"workspace && lds_split <= ([^)]+)\)"),
    "LDS_LIMIT_EXACT": (LDS_LIMIT, "kpff.hip", "gdkvm_kpff_fwd_train", r"if \(lds > ([^)]+)\) return gdkvm_fail"),
    "PAIR_MIN_TILES": (2, "kpff.hip", "gdkvm_kpff_fwd_train", r"&& total_tiles >= (\d+) && total_tiles >= single_below;"),
    "SINGLE_BELOW_OVER_CUS": (1, "kpff.hip", "gdkvm_kpff_fwd_train", r"&& n > 0\) return n \+ (\d+);"),
    "SINGLE_BELOW_FALLBACK": (257, "kpff.hip", "gdkvm_kpff_fwd_train", r"return (\d+);\s*\}\(\);"),
    "PACKED_TOKENS": (56, "kpff.hip", "gdkvm_kpff_fwd_train", r"const bool packed56 = pair && rows \* cols <= (\d+);"),
    "PACKED_SB": (56, "kpff.hip", "gdkvm_kpff_fwd_train", r"hipLaunchKernelGGL\(\(kpff_bf16_kernel<2, KPFF_OT, (\d+)>\)"),
    "PACKED_LDS_ROWS": (112, "kpff.hip", "gdkvm_kpff_fwd_train", r"packed56 \? \(size_t\)(\d+) \* \(Cin \+ KPFF_PAD16\)"),
    "BWD_PRE_BLOCKS_F32": (2048, "kpff.hip", "gdkvm_kpff_bwd_pre", r"kpff_bwd_pre_kernel<GDKVM_F32>\), dim3\((\d+)\), dim3\(\d+\)"),
    "BWD_PRE_THREADS_F32": (256, "kpff.hip", "gdkvm_kpff_bwd_pre", r"kpff_bwd_pre_kernel<GDKVM_F32>\), dim3\(\d+\), dim3\((\d+)\)"),
    "BWD_PRE_BLOCKS_BF16": (2048, "kpff.hip", "gdkvm_kpff_bwd_pre", r"kpff_bwd_pre_kernel<GDKVM_BF16>\), dim3\((\d+)\), dim3\(\d+\)"),
    "BWD_PRE_THREADS_BF16": (256, "kpff.hip", "gdkvm_kpff_bwd_pre", r"kpff_bwd_pre_kernel<GDKVM_BF16>\), dim3\(\d+\), dim3\((\d+)\)"),
    "PROJ_TM_SWITCH": (65536, "kpff.hip", None, r"constexpr int PROJ_TM_SWITCH = ([^;]+);"),
    "PROJ_TM_LARGE": (128, "kpff.hip", "gdkvm_proj_rows", r"const int TM = rows >= PROJ_TM_SWITCH \? (\d+) : \d+;"),
    "PROJ_TM_SMALL": (64, "kpff.hip", "gdkvm_proj_rows", r"const int TM = rows >= PROJ_TM_SWITCH \? \d+ : (\d+);"),
}
globals().update({k: v[0] for k, v in CONSTANTS.items()})
# Expressions the functions below restate (no single literal to read): test_kpff_forms_cpu.py pins their text.
SOURCE_LINES = (
    "if (h * w <= KPFF_TM) rows = h;",
    "else if (w <= 16) rows = (KPFF_TM / w) & ~3;",                        # whole 4-row bands: every 2x2 / 4x4 pooling cell is tile-local
    "const int col_tiles = (w + cols - 1) / cols;",
    "const int tiles = ((h + rows - 1) / rows) * col_tiles;",
    "const size_t lds1 = (size_t)KPFF_TM * (Cin + KPFF_PAD16) * sizeof(bf16_t);",
    "const size_t lds_split = (size_t)2 * KPFF_TM * (Cin + KPFF_PAD16) * sizeof(bf16_t);",
    "if (io_dtype == GDKVM_BF16 && Ck % 32 == 0 && Cv % 32 == 0 && Cp % 32 == 0) {",
    "if (io_dtype == GDKVM_F32 && Ck % 32 == 0 && Cv % 32 == 0 && Cp % 32 == 0 && workspace && lds_split <= 160 * 1024) {",
    "constexpr int NTHR = 256 * NT / OT, TMW = SB * NT, MT = (TMW + 15) / 16;",
    "constexpr int OB_STEP = 16 * OT * (NTHR / 64);",                      # output channels a workgroup's waves cover per round
    "dim3((unsigned)((total_tiles + 1) / 2)), dim3(512 / KPFF_OT), lds, st, b, total_tiles);",
    "for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {",
)


def source_constant(name, csrc=gc.CSRC):
    return gc.source_constant(name, csrc, CONSTANTS)


def _cdiv(a, b):
    return -(-a // b)


def tiling(h, w):
    """The cut of an h x w grid: a tile is `rows` grid rows x `cols` columns; `bands` lists each tile of a frame as (grid rows, width)."""
    rows, cols = None, w
    if h * w <= KPFF_TM:
        rows = h
    elif w <= FULL_WIDTH_MAX:
        rows = (KPFF_TM // w) & ~3
    else:
        rows, cols = COL_TILE_ROWS, COL_TILE_COLS
    col_tiles = _cdiv(w, cols)
    tiles = _cdiv(h, rows) * col_tiles
    bands = [(min(rows, h - r0), min(cols, w - c0)) for r0 in range(0, h, rows) for c0 in range(0, w, cols)]
    assert len(bands) == tiles and sum(a * b for a, b in bands) == h * w
    return NS(rows=rows, cols=cols, col_tiles=col_tiles, tiles=tiles, full_w=cols >= w, bands=bands, tokens=[a * b for a, b in bands])


def arm(io, ck, cv, cp, workspace=True):
    """"bf16" (bf16 MFMA arm), "split" (fp32 I/O on bf16 splits) or "exact" (fp32 MFMA), as gdkvm_kpff_fwd_train chooses."""
    aligned = ck % 32 == 0 and cv % 32 == 0 and cp % 32 == 0
    cin = cp + ck + cv
    if io == "bf16" and aligned:
        return "bf16"
    if io == "fp32" and aligned and workspace and 2 * KPFF_TM * (cin + KPFF_PAD16) * 2 <= LDS_LIMIT_SPLIT:
        return "split"
    return "exact"


def bf16_form(total_tiles, cus, tile_tokens, cin):
    """The bf16 arm's kernel for a batch of `total_tiles` tiles of at most `tile_tokens` (= rows x cols) tokens on `cus` compute units:
    form "single" (kpff_bf16_kernel<1, 1>), "pair" (<2, KPFF_OT>) or "packed56" (<2, KPFF_OT, 56>), its workgroups, threads and LDS bytes,
    the output channels its waves cover per round, and whether the last workgroup's second sub-tile is invalid."""
    lds1 = KPFF_TM * (cin + KPFF_PAD16) * 2
    if lds1 > LDS_LIMIT_TILE:
        raise ValueError("Cp + Ck + Cv = %d exceeds the LDS tile" % cin)
    pair = 2 * lds1 <= LDS_LIMIT_PAIR and total_tiles >= PAIR_MIN_TILES and total_tiles >= cus + SINGLE_BELOW_OVER_CUS
    packed = pair and tile_tokens <= PACKED_TOKENS
    nt = 2 if pair else 1
    ot = KPFF_OT if pair else 1
    nthr = 256 * nt // ot
    return NS(form="packed56" if packed else "pair" if pair else "single", blocks=_cdiv(total_tiles, nt), threads=nthr,
              lds=PACKED_LDS_ROWS * (cin + KPFF_PAD16) * 2 if packed else nt * lds1, sb=PACKED_SB if packed else KPFF_TM,
              ob_step=16 * ot * (nthr // 64), idle_second=pair and total_tiles % 2 == 1)


def threshold_bt(h, w, cus, odd=False):
    """The fewest frames of an h x w grid that reach the two-sub-tile forms on `cus` compute units; `odd`: one more where that makes the
    total tile count odd (possible only for one tile per frame)."""
    tpf = tiling(h, w).tiles
    bt = _cdiv(cus + SINGLE_BELOW_OVER_CUS, tpf)
    if odd and (bt * tpf) % 2 == 0:
        assert tpf % 2 == 1
        bt += 1
    return bt


def slices(bt, h, w, cus):
    """Frame ranges that cover 0 .. bt, each below the threshold (at most `cus` tiles), the first cut at an ODD frame."""
    per = cus // tiling(h, w).tiles
    first = per if per % 2 else per - 1
    assert first >= 1
    cuts = [0, min(first, bt)]
    while cuts[-1] < bt:
        cuts.append(min(cuts[-1] + per, bt))
    return list(zip(cuts[:-1], cuts[1:]))


def bwd_pre_trips(m, cp):
    """kpff_bwd_pre_kernel on M rows: (the most trips a thread takes, whether the last trip is partial)."""
    assert BWD_PRE_BLOCKS_F32 == BWD_PRE_BLOCKS_BF16 and BWD_PRE_THREADS_F32 == BWD_PRE_THREADS_BF16
    threads = BWD_PRE_BLOCKS_F32 * BWD_PRE_THREADS_F32
    return NS(trips=_cdiv(m * cp, threads), partial=(m * cp) % threads != 0)


def proj_tile(rows):
    return PROJ_TM_LARGE if rows >= PROJ_TM_SWITCH else PROJ_TM_SMALL


# ---------------------------------------------------------------------------------------------------------------------------------------
# The cases of tests/test_kpff_train_forms_gpu.py: (h, w), (Ck, Cv, Cp), the form the bf16 arm takes at the threshold batch, odd tile count.
CASES = {
    "a": ((7, 7), (32, 32, 64), "packed56", True),       # odd tile count, idle waves (Cp < OB_STEP)
    "b": ((7, 7), (64, 256, 256), "packed56", False),    # the default widths, two output-tile rounds per wave
    "c": ((14, 14), (32, 64, 64), "packed56", False),    # ragged last band (28 tokens)
    "d": ((14, 7), (32, 32, 32), "packed56", False),     # bands of 8 and 6 rows
    "e": ((16, 16), (64, 256, 256), "pair", False),      # 4 tiles per frame
    "f": ((6, 19), (32, 32, 64), "pair", False),         # column-tiled, full_w == false
    "g": ((21, 5), (32, 32, 32), "pair", False),         # 60-token bands
    "h": ((5, 3), (32, 32, 32), "packed56", True),       # 15-token tiles
}
SMALL_BT = 3
SAVES_BF16 = ("a", "c", "e", "f")                        # each form anchored in its single-tile version
SAVES_SPLIT = ("a", "e", "f")
SAVES_EXACT = ((5, 3, 16, 48, 80), (6, 19, 16, 16, 32))  # (h, w, Ck, Cv, Cp), both I/O dtypes
PRE_CASES = ((3, 49, 64), (257, 49, 64), (257, 49, 256))  # (BT, N, Cp): one trip, two with a partial second, seven
POST_CASES = (("a", (7, 7), (32, 32, 64)), ("c", (14, 14), (32, 64, 64)), ("f", (6, 19), (32, 32, 64)), ("g", (21, 5), (32, 32, 32)),
              ("1x1", (1, 1), (32, 32, 32)))
BACKWARD_BF16 = ("a", "e", "f")
BACKWARD_FP32 = ("a", "f")
PROJ_CASE = (65613, 64, (16, 32))
