#!/usr/bin/env python3
"""CAMUS NIfTI release -> the PNG tree gdkvm_amd.data.CamusPng reads (BASELINE.json configs[2]).

The dataset as published (the "raw data" link of the reference's guide, /root/reference/website/src/pages/[lang]/reprod/index.astro:221):
    <src>/patientXXXX/patientXXXX_<2CH|4CH>_half_sequence.nii.gz        the ED -> ES image sequence  [W, H, F]
    <src>/patientXXXX/patientXXXX_<2CH|4CH>_half_sequence_gt.nii.gz     its labels: 0 background, 1 LV, 2 myocardium, 3 left atrium
    (optionally <src>/subgroup_{training,validation,testing}.txt: one patient id per line; without them every patient goes to --split)
Written (what the reference calls "camus_png256x256_10f": 256 x 256, 10 frames per sequence -- index.astro:217,246):
    <dst>/<split>/patientXXXX/<2CH|4CH>/frame_000.png ... mask_000.png ...   `--frames` frames evenly spread over the sequence, resized
    to `--size` (images bilinear, labels nearest)
    <dst>/<split>/patientXXXX/<2CH|4CH>/spacing.json   {"spacing_um": [row_um, col_um], "native_hw": [H, W]}: the micrometres per pixel of
    the RESIZED grid, down the rows and along the columns, from the header's pixdim (pixdim[1] belongs to the stored x = width, pixdim[2] to
    y = height): row_um = rint(1000 pixdim_y_mm H / size), col_um likewise with W.  A 549 x 778 sequence squeezed to 256 x 256 has pixels of
    about 0.33 x 0.47 mm; eval.py measures volumes in mL and surface distances in mm with it.  No file (and a log line) when a pixdim is not
    finite or not positive, or a result falls outside 1..4095.
    <dst>/<split>/patientXXXX/<2CH|4CH>/info.json   when <src>/patientXXXX/Info_<2CH|4CH>.cfg exists: {"ef_percent", "edv_ml", "esv_ml",
    "ed_frame", "es_frame", "nb_frame", "frame_rate"} from its `key: value` lines (LVef or EF, LVedv, LVesv, ED, ES, NbFrame, FrameRate), null
    where a key is absent or holds no number.  The volumes and the EF there are the dataset's bi-plane Simpson values, stated per patient in
    both views' files; eval.py's `biplane` block compares against them.  The key names are written down from the two public CAMUS releases
    WITHOUT a copy at hand to check them: the parser takes keys in any letter case, ignores what it does not know and never fails on a line.

With --native-masks (off by default: the tree written without it is byte for byte the one above) every picked frame also gets
    <dst>/<split>/patientXXXX/<2CH|4CH>/native_mask_000.png ...   the label frame exactly as stored, transposed to rows = y, [H, W] uint8,
    untouched by any resize: the tracing as the experts drew it, which eval.py's `native` block (data.native_eval) compares the prediction
    with at the sequence's own size (CamusPng.native_target; spacing.json's "native_hw" is that size).

With --native-frames (off by default) every picked frame also gets
    <dst>/<split>/patientXXXX/<2CH|4CH>/native_frame_000.png ...   the image frame at its stored size, [H, W] uint8, by the same 255 / max
    scaling and clipping the resized frames get, applied to the un-resized frame: what predict.py and ops.frames_from_native take
    (CamusPng.native_frames).
With --resample area (the default is bilinear: the tree of before) frame_XXX.png is the exact-integer area (box) average of that native
    byte frame (the rule of gdkvm_frames_from_native in include/gdkvm.h) instead of the point-sampled bilinear resize: a tree converted this
    way holds exactly the bytes ops.frames_from_native produces from native_frame_XXX.png, so a model trained on it sees at prediction
    time what it saw in training.  Labels stay nearest.
With --native-spacing (off by default) every sequence also gets
    <dst>/<split>/patientXXXX/<2CH|4CH>/native_spacing.json   {"spacing_um": [row_um, col_um]}: the micrometres per pixel of the NATIVE
    frames, the header's pixdim itself: row_um = rint(1000 pixdim_y_mm), col_um = rint(1000 pixdim_x_mm) -- no resize rounds it.  What
    eval.py's native.surface block measures HD, HD95 and ASSD in mm with (CamusPng.native_spacing_um, data.native_surface_class).
    spacing.json stays as it is.  No file (and a log line) when a pixdim is not finite or not positive, or a value falls outside 1..4095.

NIfTI-1 is read here directly (a 348-byte header + a raw array, gzip around it): no nibabel in this image.  Nothing touches a GPU.

    python tools/convert_camus.py <src> <dst> [--size 256] [--frames 10] [--split train] [--native-masks] [--native-frames] [--resample area]
        [--native-spacing]
"""
import argparse
import glob
import gzip
import json
import math
import os
import struct

import numpy as np

_DTYPES = {2: np.uint8, 4: np.int16, 8: np.int32, 16: np.float32, 64: np.float64, 256: np.int8, 512: np.uint16, 768: np.uint32}


def read_nifti(path: str) -> np.ndarray:
    """The voxel array of a NIfTI-1 file (.nii or .nii.gz), indexed [x, y, z(, t)] as stored (Fortran order), scaled by scl_slope/inter."""
    raw = (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")).read()
    if len(raw) < 352:
        raise ValueError(f"{path}: too short for a NIfTI-1 header")
    end = "<" if struct.unpack("<i", raw[:4])[0] == 348 else ">"
    if struct.unpack(end + "i", raw[:4])[0] != 348 or raw[344:347] not in (b"n+1", b"ni1"):
        raise ValueError(f"{path}: not a NIfTI-1 file")
    dim = struct.unpack(end + "8h", raw[40:56])
    datatype = struct.unpack(end + "h", raw[70:72])[0]
    vox_offset = int(struct.unpack(end + "f", raw[108:112])[0])
    slope, inter = struct.unpack(end + "2f", raw[112:120])
    if datatype not in _DTYPES:
        raise ValueError(f"{path}: NIfTI datatype {datatype} is not handled")
    shape = tuple(int(d) for d in dim[1:1 + dim[0]])
    dt = np.dtype(_DTYPES[datatype]).newbyteorder(end)
    arr = np.frombuffer(raw, dt, int(np.prod(shape)), vox_offset).reshape(shape, order="F")
    if slope not in (0.0, 1.0) or inter != 0.0:
        arr = arr.astype(np.float32) * (slope if slope != 0.0 else 1.0) + inter
    return arr


_UNIT_MM = {0: 1.0, 1: 1000.0, 2: 1.0, 3: 0.001}                # xyzt_units & 7 -> millimetres per unit (0 = unknown is read as mm)
SPACING_UM_MAX = 4095


def read_nifti_pixdim_mm(path: str):
    """(dx, dy) in mm from a NIfTI-1 header: pixdim[1] (the stored x = width) and pixdim[2] (y = height), float32 at byte 76 + 4 i, scaled
    by the spatial unit in the low 3 bits of xyzt_units (byte 123).  The values are returned as they are: the caller checks them."""
    with (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")) as f:
        raw = f.read(352)
    if len(raw) < 348:
        raise ValueError(f"{path}: too short for a NIfTI-1 header")
    end = "<" if struct.unpack("<i", raw[:4])[0] == 348 else ">"
    dx, dy = struct.unpack(end + "2f", raw[80:88])
    unit = _UNIT_MM.get(raw[123] & 7, 1.0)
    return float(dx) * unit, float(dy) * unit


def spacing_um(dx_mm: float, dy_mm: float, native_h: int, native_w: int, size: int):
    """[row_um, col_um] of a native_h x native_w frame with pixels of dy_mm x dx_mm resized to size x size, or None when a pixdim is not
    finite or not positive or a result falls outside 1..SPACING_UM_MAX."""
    if not (math.isfinite(dx_mm) and math.isfinite(dy_mm) and dx_mm > 0 and dy_mm > 0):
        return None
    row, col = float(np.rint(1000.0 * dy_mm * native_h / size)), float(np.rint(1000.0 * dx_mm * native_w / size))
    if not (1 <= row <= SPACING_UM_MAX and 1 <= col <= SPACING_UM_MAX):
        return None
    return [int(row), int(col)]


def native_spacing_um(dx_mm: float, dy_mm: float):
    """[row_um, col_um] of the native pixel of dy_mm x dx_mm, or None when a pixdim is not finite or not positive or a value falls outside
    1..SPACING_UM_MAX."""
    if not (math.isfinite(dx_mm) and math.isfinite(dy_mm) and dx_mm > 0 and dy_mm > 0):
        return None
    row, col = float(np.rint(1000.0 * dy_mm)), float(np.rint(1000.0 * dx_mm))
    if not (1 <= row <= SPACING_UM_MAX and 1 <= col <= SPACING_UM_MAX):
        return None
    return [int(row), int(col)]


# info.json's fields and the cfg keys (lower case) each is read from, the first present one that parses wins
_INFO_KEYS = (("ef_percent", ("lvef", "ef"), float), ("edv_ml", ("lvedv",), float), ("esv_ml", ("lvesv",), float),
              ("ed_frame", ("ed", "ed_frame"), int), ("es_frame", ("es", "es_frame"), int), ("nb_frame", ("nbframe", "nb_frame"), int),
              ("frame_rate", ("framerate", "frame_rate"), float))


def parse_info_cfg(text: str) -> dict:
    """The fields of info.json from the text of a CAMUS Info_<view>.cfg: `key: value` lines, keys in any letter case, unknown keys and lines
    without a colon ignored; a field is None where none of its keys is present with a finite number (an integer field takes a whole number
    only).  The key names (LVef / EF, LVedv, LVesv, ED, ES, NbFrame, FrameRate) are from memory of the two public releases and could not be
    checked against a copy: hence the tolerance, and None rather than an error for anything unexpected."""
    seen = {}
    for line in text.splitlines():
        key, sep, val = line.partition(":")
        if sep and key.strip():
            seen.setdefault(key.strip().lower(), val.strip())
    out = {}
    for field, keys, kind in _INFO_KEYS:
        out[field] = None
        for k in keys:
            try:
                v = float(seen[k])
            except (KeyError, ValueError):
                continue
            if not math.isfinite(v) or (kind is int and v != int(v)):
                continue
            out[field] = int(v) if kind is int else v
            break
    return out


def write_nifti(path: str, arr: np.ndarray, pixdim=None) -> None:
    """A minimal NIfTI-1 writer (tests build tiny CAMUS-shaped trees with it).  pixdim = (dx, dy) in mm goes to pixdim[1..2] with the spatial
    unit set to mm; without it those header bytes stay zero, as before."""
    code = {np.dtype(v): k for k, v in _DTYPES.items()}[arr.dtype]
    hdr = bytearray(352)
    struct.pack_into("<i", hdr, 0, 348)
    struct.pack_into("<8h", hdr, 40, arr.ndim, *(list(arr.shape) + [1] * (7 - arr.ndim)))
    struct.pack_into("<h", hdr, 70, code)
    struct.pack_into("<h", hdr, 72, arr.dtype.itemsize * 8)
    if pixdim is not None:
        struct.pack_into("<2f", hdr, 80, float(pixdim[0]), float(pixdim[1]))
        hdr[123] = 2
    struct.pack_into("<f", hdr, 108, 352.0)
    struct.pack_into("<2f", hdr, 112, 1.0, 0.0)
    hdr[344:348] = b"n+1\0"
    data = bytes(hdr) + np.asfortranarray(arr).tobytes(order="F")
    (gzip.open(path, "wb") if path.endswith(".gz") else open(path, "wb")).write(data)


def resize(img: np.ndarray, size: int, nearest: bool) -> np.ndarray:
    """[H, W] -> [size, size]; half-pixel-centre sampling; bilinear for images, nearest for label maps."""
    h, w = img.shape
    ys = (np.arange(size) + 0.5) * h / size - 0.5
    xs = (np.arange(size) + 0.5) * w / size - 0.5
    if nearest:
        yi = np.clip(np.round(ys).astype(int), 0, h - 1)
        xi = np.clip(np.round(xs).astype(int), 0, w - 1)
        return img[yi][:, xi]
    y0 = np.clip(np.floor(ys).astype(int), 0, h - 1); y1 = np.clip(y0 + 1, 0, h - 1); fy = np.clip(ys - y0, 0, 1)[:, None]
    x0 = np.clip(np.floor(xs).astype(int), 0, w - 1); x1 = np.clip(x0 + 1, 0, w - 1); fx = np.clip(xs - x0, 0, 1)[None, :]
    f = img.astype(np.float32)
    top = f[y0][:, x0] * (1 - fx) + f[y0][:, x1] * fx
    bot = f[y1][:, x0] * (1 - fx) + f[y1][:, x1] * fx
    return top * (1 - fy) + bot * fy


def native_bytes(img: np.ndarray) -> np.ndarray:
    """[H, W] of any dtype -> uint8 [H, W]: the scaling and clipping the resized frames get (255 / max when the maximum exceeds 255),
    applied to the frame at its stored size."""
    a = img.astype(np.float32)
    hi = float(a.max()) or 1.0
    return np.clip(a * (255.0 / hi if hi > 255.0 else 1.0), 0, 255).astype(np.uint8)


def _area_weights(n_grid: int, n_native: int) -> np.ndarray:
    i = np.arange(n_grid, dtype=np.int64)[:, None]
    k = np.arange(n_native, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((i + 1) * n_native, (k + 1) * n_grid) - np.maximum(i * n_native, k * n_grid))


def resize_area(v: np.ndarray, size: int) -> np.ndarray:
    """uint8 [H, W] -> uint8 [size, size] by the exact-integer area (box) average of gdkvm_frames_from_native (include/gdkvm.h): the
    overlap weights of the two pixel lattices, N = Wy v Wx^T in int64, q = floor((2 N + H W) / (2 H W)) -- the bytes
    ops.frames_from_native produces from the same frame."""
    if v.dtype != np.uint8 or v.ndim != 2:
        raise ValueError(f"resize_area takes a uint8 [H, W] frame, got {v.dtype} {v.shape}")
    h, w = v.shape
    n = _area_weights(size, h) @ v.astype(np.int64) @ _area_weights(size, w).T
    return ((2 * n + h * w) // (2 * h * w)).astype(np.uint8)


def _splits(src: str, default: str) -> dict:
    out = {}
    for name, split in (("training", "train"), ("validation", "val"), ("testing", "test")):
        p = os.path.join(src, f"subgroup_{name}.txt")
        if os.path.exists(p):
            for line in open(p):
                if line.strip():
                    out[line.strip()] = split
    return out if out else defaultdict_const(default)


class defaultdict_const(dict):
    def __init__(self, v):
        super().__init__()
        self.v = v

    def get(self, k, d=None):
        return self.v


def convert(src: str, dst: str, size: int = 256, frames: int = 10, split: str = "train", log=print, native_masks: bool = False,
            native_frames: bool = False, resample: str = "bilinear", native_spacing: bool = False) -> dict:
    from PIL import Image
    if resample not in ("bilinear", "area"):
        raise ValueError(f"resample = {resample!r} is neither 'bilinear' nor 'area'")
    splits = _splits(src, split)
    done = infos = 0
    for pdir in sorted(glob.glob(os.path.join(src, "patient*"))):
        pid = os.path.basename(pdir)
        for view in ("2CH", "4CH"):
            seq = [p for e in (".nii.gz", ".nii") for p in glob.glob(os.path.join(pdir, f"{pid}_{view}_half_sequence{e}"))]
            gt = [p for e in (".nii.gz", ".nii") for p in glob.glob(os.path.join(pdir, f"{pid}_{view}_half_sequence_gt{e}"))]
            if not seq or not gt:
                continue
            img, lab = read_nifti(seq[0]), read_nifti(gt[0])                  # [W, H, F] each
            if img.shape != lab.shape or img.ndim != 3:
                log(f"  skipped {pid} {view}: image {img.shape} against labels {lab.shape}")
                continue
            out = os.path.join(dst, splits.get(pid, split), pid, view)
            os.makedirs(out, exist_ok=True)
            pick = np.round(np.linspace(0, img.shape[2] - 1, frames)).astype(int) if img.shape[2] >= frames else np.arange(img.shape[2])
            for j, f in enumerate(pick):
                a = resize(np.asarray(img[:, :, f]).T, size, False)           # stored [x, y] -> rows = y
                m = resize(np.asarray(lab[:, :, f]).T.astype(np.int64), size, True)
                hi = float(a.max()) or 1.0
                fr = np.clip(a * (255.0 / hi if hi > 255.0 else 1.0), 0, 255).astype(np.uint8)
                if native_frames or resample == "area":
                    nb = native_bytes(np.asarray(img[:, :, f]).T)             # the image frame at its stored size, as bytes
                    if resample == "area":                                    # the bytes ops.frames_from_native makes of native_frame_XXX.png
                        fr = resize_area(nb, size)
                    if native_frames:
                        Image.fromarray(np.ascontiguousarray(nb)).save(os.path.join(out, f"native_frame_{j:03d}.png"))
                Image.fromarray(fr).save(os.path.join(out, f"frame_{j:03d}.png"))
                Image.fromarray(m.astype(np.uint8)).save(os.path.join(out, f"mask_{j:03d}.png"))
                if native_masks:                                              # the labels as stored: no resize of any kind
                    Image.fromarray(np.ascontiguousarray(np.asarray(lab[:, :, f]).T).astype(np.uint8)).save(os.path.join(out, f"native_mask_{j:03d}.png"))
            dx_mm, dy_mm = read_nifti_pixdim_mm(seq[0])
            sp = spacing_um(dx_mm, dy_mm, img.shape[1], img.shape[0], size)
            if sp is None:
                log(f"  {pid} {view}: no usable pixel spacing (pixdim {dx_mm} x {dy_mm} mm, native {img.shape[1]} x {img.shape[0]}): no spacing.json")
            else:
                with open(os.path.join(out, "spacing.json"), "w") as f:
                    json.dump({"spacing_um": sp, "native_hw": [int(img.shape[1]), int(img.shape[0])]}, f)
            if native_spacing:                                                # the pixdim itself: the spacing of the native frames
                nsp = native_spacing_um(dx_mm, dy_mm)
                if nsp is None:
                    log(f"  {pid} {view}: no usable native pixel spacing (pixdim {dx_mm} x {dy_mm} mm): no native_spacing.json")
                else:
                    with open(os.path.join(out, "native_spacing.json"), "w") as f:
                        json.dump({"spacing_um": nsp}, f)
            cfg = os.path.join(pdir, f"Info_{view}.cfg")
            if os.path.exists(cfg):
                with open(cfg, errors="replace") as f:
                    info = parse_info_cfg(f.read())
                with open(os.path.join(out, "info.json"), "w") as f:
                    json.dump(info, f)
                infos += 1
            done += 1
    log(f"converted {done} sequences ({infos} with an info.json)")
    return {"sequences": done}


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--split", default="train")
    ap.add_argument("--native-masks", action="store_true", help="also write every picked label frame at its own size (native_mask_XXX.png)")
    ap.add_argument("--native-frames", action="store_true", help="also write every picked image frame at its own size as bytes (native_frame_XXX.png)")
    ap.add_argument("--resample", choices=("bilinear", "area"), default="bilinear",
                    help="how frame_XXX.png is made: point-sampled bilinear (the default), or the exact area average of ops.frames_from_native")
    ap.add_argument("--native-spacing", action="store_true",
                    help="also write the spacing of the native pixel, the header's pixdim in micrometres (native_spacing.json)")
    a = ap.parse_args()
    convert(a.src, a.dst, a.size, a.frames, a.split, native_masks=a.native_masks, native_frames=a.native_frames, resample=a.resample,
            native_spacing=a.native_spacing)
