"""Clip datasets for the harness.  No dataset ships with this repository and there is no network,
so the default is a seeded synthetic echo-like clip generator; two on-disk formats are supported for real data:

  npy_clips    <root>/<split>/<name>.npz with  frames [T,H,W] or [T,H,W,3] uint8  and  masks [T,H,W] uint8
  echonet_npz  what tools/convert_echonet.py writes from an EchoNet-Dynamic download (Videos/*.avi, FileList.csv, VolumeTracings.csv --
               the "raw data" link of the reference's guide, website reprod/index.astro:222): one .npz per video with the WHOLE video and
               the two traced frames' masks; EchoNetNpz cuts a T-frame clip around the traced frames and marks every other frame
               UNLABELLED (label 255, which the loss leaves out: gdkvm_amd.train.segmentation_loss, gdkvm_seg_loss_fwd); with
               data.whole_video the clip is the video's first T frames instead (several heart beats: what ops.lv_beats is for), and the
               optional scalars `ef` (FileList.csv's EF in per cent) and `fps` serve as a second reference
  camus_png    <root>/<split>/<patient>/<view>/frame_XXX.png + mask_XXX.png, view in {2CH, 4CH}, masks 0 bg / 1 LV / 2 myocardium / 3 LA --
               what tools/convert_camus.py writes from the CAMUS NIfTI release (guide: index.astro:221); the reference's own processed
               "camus_png256x256_10f" tree is not documented beyond its name (index.astro:217,246), so this layout is the builder's;
               beside the PNGs an optional spacing.json {"spacing_um": [row_um, col_um], "native_hw": [H, W]}: the pixel spacing of the
               RESIZED grid in micrometres, from the NIfTI pixdim, and an optional info.json with the EF and volumes the release states for
               the patient (CamusPng.info); view_pair_table pairs a patient's two views for the bi-plane volume (ops.lv_biplane)

A dataset's spacing_um(i) is clip i's pixel spacing (row_um, col_um) in integer micrometres per pixel of the grid its masks are on, or None;
clip_spacing_table gathers them for eval.py, which then reports volumes in mL and surface distances in mm.  A dataset's length(i), where it has
one, is the number of clip i's frames that come from the video (the rest repeats the last frame); clip_length_table gathers those for
ops.lv_beats.  A dataset's native_hw(i) / native_target(i), where it has them (npy_clips: an optional `native_target` array [T, h0, w0] in the
.npz; camus_png: the native_mask_XXX.png of tools/convert_camus.py --native-masks), are clip i's labels at the clip's OWN frame size, untouched
by any resize; native_target_table gathers the sizes for eval.py's `native` block (data.native_eval).  native_frames(i) likewise hands out the
clip's grey IMAGE frames at their own size (npy_clips: an optional `native_frames` array; camus_png: the native_frame_XXX.png of
tools/convert_camus.py --native-frames), what ops.frames_from_native and predict.py take.  native_spacing_um(i) is the spacing of the
NATIVE pixel (npy_clips: an optional `native_spacing_um` array; camus_png: the native_spacing.json of tools/convert_camus.py
--native-spacing), else None; native_spacing_table gathers them, with `data.native_spacing_um` as the fallback, for the surface distances at
native size (ops.surface_distance_native, eval.py's native.surface block).  Samples stay (frames, target).
"""
from __future__ import annotations

import glob
import json
import os
from typing import Optional, Tuple

import numpy as np
import torch
from torch.utils.data import Dataset


SPACING_UM_MAX = 4095


def _spacing_pair(v) -> Optional[Tuple[int, int]]:
    """(row_um, col_um) when v holds two integers in 1..SPACING_UM_MAX, else None."""
    try:
        a = np.asarray(v)
        if a.shape != (2,) or not np.issubdtype(a.dtype, np.integer):
            return None
        ry, rx = int(a[0]), int(a[1])
    except (TypeError, ValueError):
        return None
    return (ry, rx) if 1 <= ry <= SPACING_UM_MAX and 1 <= rx <= SPACING_UM_MAX else None


class SyntheticEchoClips(Dataset):
    """Speckled clips with a pulsating ellipse ("ventricle") and, for >2 classes, concentric wall / atrium regions.
    Deterministic per index, so ranks and epochs are reproducible.  A clip holds `beats` periods of the pulsation (1.0: exactly one, the
    clips of before bit for bit).  With a whole number of beats >= 2 the clip is meant to SHOW that many beats: the phase is drawn so that
    every period's smallest area keeps 0.3 periods from both ends of the clip -- a minimum nearer than a quarter period to an end has less than
    half the curve's range beside it and is no end-systole for ops.lv_beats (nor a peak for scipy.signal.find_peaks) at the usual prominence
    of 0.5.  Every other value of `beats` keeps the free phase."""

    def __init__(self, n_clips: int, frames: int, size: int, num_classes: int = 2, seed: int = 0, as_uint8: bool = False, beats: float = 1.0):
        if not float(beats) > 0:
            raise ValueError(f"SyntheticEchoClips: beats = {beats!r} must be > 0")
        self.n, self.T, self.S, self.C, self.seed, self.as_uint8 = n_clips, frames, size, num_classes, seed, as_uint8
        self.beats = float(beats)

    def __len__(self):
        return self.n

    def spacing_um(self, i):
        return None                                               # a drawing has no physical size

    def native_spacing_um(self, i):
        return None

    def __getitem__(self, i) -> Tuple[torch.Tensor, torch.Tensor]:
        rng = np.random.default_rng(self.seed * 1_000_003 + i)
        S, T = self.S, self.T
        yy, xx = np.mgrid[0:S, 0:S].astype(np.float32)
        cy, cx = S * (0.45 + 0.1 * rng.random()), S * (0.45 + 0.1 * rng.random())
        ry0, rx0 = S * (0.22 + 0.06 * rng.random()), S * (0.15 + 0.05 * rng.random())
        u = rng.random()
        phase, rate = u * 2 * np.pi, 2 * np.pi * self.beats / max(T, 2)
        if self.beats >= 2 and self.beats == int(self.beats):
            # the minima are where phase + rate t = 3 pi / 2 (mod 2 pi): the first at t0 in [0.3 P, 0.7 P - 1], P = the period in frames, so
            # that the last, t0 + (beats - 1) P, ends 0.3 P in front of frame T - 1
            period = max(T, 2) / self.beats
            phase = 1.5 * np.pi - rate * (0.3 * period + u * max(0.4 * period - 1.0, 0.0))
        frames = np.empty((T, 3, S, S), np.float32)
        masks = np.zeros((T, S, S), np.uint8)
        for t in range(T):
            k = 1.0 + 0.18 * np.sin(phase + rate * t)
            d = ((yy - cy) / (ry0 * k)) ** 2 + ((xx - cx) / (rx0 * k)) ** 2
            m = np.zeros((S, S), np.uint8)
            if self.C > 2:
                m[d < 1.45] = 2                                   # myocardium ring
            m[d < 1.0] = 1                                        # cavity
            if self.C > 3:
                m[(((yy - cy - 1.6 * ry0) / (0.6 * ry0)) ** 2 + ((xx - cx) / (1.1 * rx0)) ** 2) < 1.0] = 3   # atrium
            tissue = 0.55 - 0.4 * (m == 1) + 0.15 * (m == 2)
            speckle = np.sqrt(-2.0 * np.log(np.clip(rng.random((S, S)), 1e-7, 1.0))) * 0.25      # Rayleigh
            img = np.clip(tissue * speckle * 1.6, 0, 1).astype(np.float32)
            frames[t] = img[None]
            masks[t] = m
        if self.as_uint8:                                         # bytes, as a video decoder would hand them over (as_uint8: see build_dataset)
            return torch.from_numpy(np.round(frames * 255.0).astype(np.uint8)), torch.from_numpy(masks)
        return torch.from_numpy(frames), torch.from_numpy(masks.astype(np.int64))


IGNORE_LABEL = 255             # an unlabelled pixel / frame: outside [0, num_classes), so the loss and the Dice counts skip it


IDENTITY_ROW = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0)


class ClipAugment:
    """Samples the per-clip parameter rows of ops.augment_clips (gdkvm_augment_clips): one affine warp and one intensity curve per clip, the
    same for every frame of it.  The kernel warps while it casts the bytes to [0, 1] on the device (pipeline.DevicePrefetcher(augment=...));
    nothing is warped on the host -- this class only draws 8 numbers per clip and composes a 2 x 3 matrix.

      rotate_deg   rotation about the frame centre, uniform in [-rotate_deg, +rotate_deg] degrees
      scale        (lo, hi): isotropic zoom about the frame centre, uniform (> 1 enlarges the content)
      translate    shift, uniform in [-translate, +translate] as a fraction of the frame's width (x) and height (y)
      hflip        probability of a left-right mirror about the frame centre
      gain, gamma  (lo, hi): out = gain * in ** gamma + bias on intensities in [0, 1], clamped; gain uniform, gamma log-uniform
      bias         uniform in [-bias, +bias]

    Forward map of a source pixel index p = (x, y) (x to the right, y down, pixel centres at integers), c = ((W-1)/2, (H-1)/2):
        p' = A (p - c) + c + (tx W, ty H),   A = scale * [[cos a, -sin a], [sin a, cos a]] * diag(-1 if mirrored else 1, 1)
    A row holds the INVERSE of it (destination -> source: what a gather needs), inverted in float64 and stored as fp32, then gain, bias,
    gamma and three zeros.  The defaults are all no-ops: the rows are then exactly IDENTITY_ROW.
    params() draws from np.random.default_rng([seed, rank, epoch, index]): the same arguments give the same rows, ranks and batches differ,
    and a run resumed at an epoch repeats that epoch's sequence (the granularity at which train.py resumes the shuffle)."""

    def __init__(self, rotate_deg: float = 0.0, scale=(1.0, 1.0), translate: float = 0.0, hflip: float = 0.0, gain=(1.0, 1.0),
                 bias: float = 0.0, gamma=(1.0, 1.0), seed: int = 0, rank: int = 0):
        pair = lambda v: (float(v[0]), float(v[1]))
        self.rotate_deg, self.translate, self.hflip, self.bias = float(rotate_deg), float(translate), float(hflip), float(bias)
        self.scale, self.gain, self.gamma = pair(scale), pair(gain), pair(gamma)
        self.seed, self.rank = int(seed), int(rank)
        for name, (lo, hi) in (("scale", self.scale), ("gain", self.gain), ("gamma", self.gamma)):
            if not lo <= hi:
                raise ValueError(f"ClipAugment: {name} range ({lo}, {hi}) is not (lo, hi)")
        if self.scale[0] <= 0 or self.gamma[0] <= 0:
            raise ValueError("ClipAugment: scale and gamma must be positive")
        if self.rotate_deg < 0 or self.translate < 0 or self.bias < 0 or not 0.0 <= self.hflip <= 1.0:
            raise ValueError("ClipAugment: rotate_deg, translate and bias are magnitudes (>= 0), hflip a probability")
        if self.seed < 0 or self.rank < 0:
            raise ValueError("ClipAugment: seed and rank must be non-negative")

    def draw(self, epoch: int, index: int, B: int) -> dict:
        """The raw draws of batch `index` of `epoch`, float64 arrays of length B (always all eight, in this order, whatever the ranges)."""
        rng = np.random.default_rng([self.seed, self.rank, int(epoch), int(index)])
        return {"angle_deg": rng.uniform(-self.rotate_deg, self.rotate_deg, B),
                "scale": rng.uniform(self.scale[0], self.scale[1], B),
                "tx": rng.uniform(-self.translate, self.translate, B),
                "ty": rng.uniform(-self.translate, self.translate, B),
                "flip": rng.random(B) < self.hflip,
                "gain": rng.uniform(self.gain[0], self.gain[1], B),
                "bias": rng.uniform(-self.bias, self.bias, B),
                "gamma": np.exp(rng.uniform(np.log(self.gamma[0]), np.log(self.gamma[1]), B))}

    def params(self, epoch: int, index: int, B: int, H: int, W: int) -> torch.Tensor:
        """fp32 [B, 12] host tensor: the rows of batch `index` of `epoch` for frames of H x W pixels."""
        d = self.draw(epoch, index, B)
        c = np.array([(W - 1) / 2.0, (H - 1) / 2.0])
        a = np.deg2rad(d["angle_deg"])
        cos, sin, mirror = np.cos(a), np.sin(a), np.where(d["flip"], -1.0, 1.0)
        fwd = np.zeros((B, 3, 3))
        fwd[:, 0, 0], fwd[:, 0, 1], fwd[:, 1, 0], fwd[:, 1, 1] = cos * mirror, -sin, sin * mirror, cos
        fwd[:, :2, :2] *= d["scale"][:, None, None]
        fwd[:, :2, 2] = c + np.stack([d["tx"] * W, d["ty"] * H], 1) - fwd[:, :2, :2] @ c
        fwd[:, 2, 2] = 1.0
        rows = np.zeros((B, 12), np.float64)
        rows[:, :6] = np.linalg.inv(fwd)[:, :2].reshape(B, 6)
        rows[:, 6], rows[:, 7], rows[:, 8] = d["gain"], d["bias"], d["gamma"]
        return torch.from_numpy((rows + 0.0).astype(np.float32))


def build_augment(cfg, rank: int = 0):
    """The ClipAugment of a run configuration (config.AugmentCfg), or None when augmentation is off."""
    a = cfg.augment
    if not a.enabled:
        return None
    return ClipAugment(rotate_deg=a.rotate_deg, scale=a.scale, translate=a.translate, hflip=a.hflip, gain=a.gain, bias=a.bias,
                       gamma=a.gamma, seed=cfg.seed, rank=rank)


def polygon_mask(xs, ys, height: int, width: int) -> np.ndarray:
    """uint8 [height, width] mask of the closed polygon (xs[i], ys[i]) -- even-odd scanline fill at pixel centres, vertices in pixel
    coordinates (x to the right, y down), as the EchoNet tracings are given.  Pure numpy: the converter runs without skimage / cv2."""
    xs, ys = np.asarray(xs, np.float64), np.asarray(ys, np.float64)
    mask = np.zeros((height, width), np.uint8)
    n = len(xs)
    if n < 3:
        return mask
    x0, y0, x1, y1 = xs, ys, np.roll(xs, -1), np.roll(ys, -1)
    cols = np.arange(width) + 0.0
    for r in range(max(0, int(np.floor(ys.min()))), min(height, int(np.ceil(ys.max())) + 1)):
        yc = r + 0.0
        cross = (y0 <= yc) != (y1 <= yc)                     # edges that straddle the scanline (half-open: a vertex counts once)
        if not cross.any():
            continue
        xi = np.sort(x0[cross] + (yc - y0[cross]) * (x1[cross] - x0[cross]) / (y1[cross] - y0[cross]))
        inside = np.zeros(width, bool)
        for a, b in zip(xi[0::2], xi[1::2]):
            inside |= (cols >= a) & (cols <= b)
        mask[r] = inside
    return mask


def echonet_tracing_polygon(rows):
    """The polygon of one traced frame from its VolumeTracings.csv rows [(X1, Y1, X2, Y2), ...]: row 0 is the long axis, every
    following row one chord across the ventricle; the outline runs down the chords' first end points and back up their second ones
    (the construction EchoNet-Dynamic's own loader uses [LIT])."""
    r = np.asarray(rows, np.float64)
    x = np.concatenate([r[1:, 0], r[1:, 2][::-1]])
    y = np.concatenate([r[1:, 1], r[1:, 3][::-1]])
    return x, y


def clip_indices(n_frames: int, labelled, T: int, pad: int = 2) -> np.ndarray:
    """T frame indices of a clip that CONTAINS every labelled frame (EchoNet: ED and ES), evenly spread from a little before the first to
    a little after the last (deterministic); videos shorter than T repeat their last frame."""
    lab = sorted(int(i) for i in labelled)
    lo, hi = max(0, lab[0] - pad), min(n_frames - 1, lab[-1] + pad)
    if hi - lo + 1 < T:                                     # widen the window to T frames where the video allows
        grow = T - (hi - lo + 1)
        lo = max(0, lo - grow // 2)
        hi = min(n_frames - 1, lo + T - 1)
        lo = max(0, hi - T + 1)
    idx = np.round(np.linspace(lo, hi, T)).astype(np.int64)
    taken = set()
    for f in lab:                                           # every labelled frame sits in the clip, each on its own position
        order = np.argsort(np.abs(idx - f), kind="stable")
        j = next(int(o) for o in order if int(o) not in taken)
        idx[j] = f
        taken.add(j)
    return np.sort(idx)


class EchoNetNpz(Dataset):
    """EchoNet-Dynamic as tools/convert_echonet.py leaves it: <root>/<split>/<FileName>.npz with `video` [F,H,W] uint8 (grey),
    `traced` [2] frame indices and `masks` [2,H,W] uint8 (0 background, 1 left ventricle).  A sample is a T-frame clip around the two
    traced frames: frames [T,3,H,W] float in [0,1], labels [T,H,W] int64 with IGNORE_LABEL on every untraced frame.  whole=True: the clip
    is frames 0 .. T - 1 of the video instead (a shorter video repeats its last frame; length(i) = min(F, T) says how many are its own), and a
    traced frame at or beyond T is not part of it.  Files may carry the scalars `ef` (per cent) and `fps` (file_ef, file_fps)."""

    def __init__(self, root: str, split: str, frames: int, as_uint8: bool = False, whole: bool = False):
        self.files = sorted(glob.glob(os.path.join(root, split, "*.npz")))
        if not self.files:
            raise FileNotFoundError(f"no converted EchoNet videos (.npz) under {os.path.join(root, split)}: run tools/convert_echonet.py")
        self.T, self.as_uint8, self.whole = frames, as_uint8, bool(whole)

    def __len__(self):
        return len(self.files)

    def spacing_um(self, i):
        return None                                               # EchoNet-Dynamic ships no pixel spacing

    def native_spacing_um(self, i):
        return None

    def _scalar(self, i, key) -> Optional[float]:
        with np.load(self.files[i]) as z:
            if key not in z.files:
                return None
            v = float(np.asarray(z[key]).reshape(-1)[0])
        return v if np.isfinite(v) else None

    def file_ef(self, i) -> Optional[float]:
        """FileList.csv's EF of video i in per cent, or None for a file converted without it."""
        return self._scalar(i, "ef")

    def file_fps(self, i) -> Optional[float]:
        return self._scalar(i, "fps")

    def length(self, i) -> int:
        """The frames of clip i that are the video's own: T for a window around the tracings (it may repeat frames, but holds one beat by
        construction), min(F, T) for a whole video (its last frame repeats behind that)."""
        if not self.whole:
            return self.T
        with np.load(self.files[i]) as z:
            return min(int(z["video"].shape[0]), self.T)

    def __getitem__(self, i):
        z = np.load(self.files[i])
        video, traced, masks = z["video"], z["traced"], z["masks"]
        idx = np.minimum(np.arange(self.T), video.shape[0] - 1) if self.whole else clip_indices(video.shape[0], traced, self.T)
        clip = np.ascontiguousarray(video[idx])
        x = torch.from_numpy(clip if self.as_uint8 else clip.astype(np.float32) / 255.0).unsqueeze(1).expand(-1, 3, -1, -1).contiguous()
        y = torch.full((self.T,) + video.shape[1:], IGNORE_LABEL, dtype=torch.uint8 if self.as_uint8 else torch.int64)
        for f, m in zip(traced, masks):
            if self.whole and int(f) >= self.T:                   # behind the cut: not part of this clip
                continue
            y[int(f) if self.whole else int(np.nonzero(idx == int(f))[0][0])] = torch.from_numpy(m.astype(np.uint8 if self.as_uint8 else np.int64))
        return x, y


class NpzClips(Dataset):
    def __init__(self, root: str, split: str, frames: int, as_uint8: bool = False):
        self.files = sorted(glob.glob(os.path.join(root, split, "*.npz")))
        if not self.files:
            raise FileNotFoundError(f"no .npz clips under {os.path.join(root, split)}")
        self.T, self.as_uint8 = frames, as_uint8

    def __len__(self):
        return len(self.files)

    def spacing_um(self, i):
        """The clip's optional `spacing_um` array [row_um, col_um]; None without it or when it is no pair of integers in 1..4095."""
        with np.load(self.files[i]) as z:
            return _spacing_pair(z["spacing_um"]) if "spacing_um" in z.files else None

    def native_spacing_um(self, i):
        """The clip's optional `native_spacing_um` array [row_um, col_um], the micrometres per pixel of its native frames; None without it
        or when it is no pair of integers in 1..4095."""
        with np.load(self.files[i]) as z:
            return _spacing_pair(z["native_spacing_um"]) if "native_spacing_um" in z.files else None

    def native_hw(self, i) -> Optional[Tuple[int, int]]:
        """(h0, w0) of the clip's optional `native_target` array [T, h0, w0]; None without it."""
        t = self.native_target(i)
        return None if t is None else (int(t.shape[1]), int(t.shape[2]))

    def native_target(self, i) -> Optional[torch.Tensor]:
        """The clip's optional `native_target` array, uint8 [T, h0, w0] (its first T frames): the labels at the clip's own size, 255 =
        unlabelled; None without it or when it is no 3-D array of at least T frames."""
        with np.load(self.files[i]) as z:
            if "native_target" not in z.files:
                return None
            a = z["native_target"]
        if a.ndim != 3 or a.shape[0] < self.T or not np.issubdtype(a.dtype, np.integer):
            return None
        return torch.from_numpy(np.ascontiguousarray(a[: self.T], dtype=np.uint8))

    def native_frames(self, i) -> Optional[torch.Tensor]:
        """The clip's optional `native_frames` array, uint8 [T, h0, w0] (its first T frames): the grey image frames at the clip's own size
        (what ops.frames_from_native and predict.py take); None without it or when it is no 3-D uint8 array of at least T frames."""
        with np.load(self.files[i]) as z:
            if "native_frames" not in z.files:
                return None
            a = z["native_frames"]
        if a.ndim != 3 or a.shape[0] < self.T or a.dtype != np.uint8:
            return None
        return torch.from_numpy(np.ascontiguousarray(a[: self.T]))

    def __getitem__(self, i):
        z = np.load(self.files[i])
        fr, mk = z["frames"][: self.T], z["masks"][: self.T]
        if fr.ndim == 3:
            fr = np.repeat(fr[..., None], 3, -1)
        if self.as_uint8:
            return torch.from_numpy(np.ascontiguousarray(fr, dtype=np.uint8)).permute(0, 3, 1, 2).contiguous(), torch.from_numpy(mk.astype(np.uint8))
        x = torch.from_numpy(fr.astype(np.float32) / 255.0).permute(0, 3, 1, 2).contiguous()
        return x, torch.from_numpy(mk.astype(np.int64))


class CamusPng(Dataset):
    """CAMUS sequences as PNG trees (tools/convert_camus.py): <root>/<split>/<patient>/<view>/frame_XXX.png + mask_XXX.png with view in
    {2CH, 4CH} (both chamber views are samples of their own, BASELINE.json configs[2]); masks hold class indices 0..3; a frame without a
    mask file is unlabelled (IGNORE_LABEL).  Sequences longer than `frames` are subsampled evenly, shorter ones repeat their last frame."""

    VIEWS = ("2CH", "4CH")

    def __init__(self, root: str, split: str, frames: int, views=VIEWS, as_uint8: bool = False):
        from PIL import Image                                     # noqa: F401  (fail early if Pillow is missing)
        self.as_uint8 = as_uint8
        self.seqs = sorted(d for d in glob.glob(os.path.join(root, split, "*", "*")) if os.path.isdir(d) and os.path.basename(d) in views)
        if not self.seqs:
            raise FileNotFoundError(f"no <patient>/<{'|'.join(views)}> folders under {os.path.join(root, split)}")
        self.T = frames

    def __len__(self):
        return len(self.seqs)

    def view(self, i) -> str:
        return os.path.basename(self.seqs[i])

    def patient(self, i) -> str:
        """The name of the patient folder sequence i lies in: the 2CH and the 4CH sequence of a patient share it (view_pair_table)."""
        return os.path.basename(os.path.dirname(self.seqs[i]))

    def info(self, i) -> Optional[dict]:
        """The sequence's info.json (tools/convert_camus.py, from the release's Info_<view>.cfg): a dict with ef_percent, edv_ml, esv_ml (the
        dataset's bi-plane Simpson values of the patient), ed_frame, es_frame, nb_frame, frame_rate, each a number or None; None without the
        file or when it holds no JSON object."""
        p = os.path.join(self.seqs[i], "info.json")
        if not os.path.exists(p):
            return None
        try:
            with open(p) as f:
                d = json.load(f)
        except ValueError:
            return None
        return d if isinstance(d, dict) else None

    def spacing_um(self, i):
        """The sequence's spacing.json "spacing_um" [row_um, col_um] (tools/convert_camus.py, from the NIfTI pixdim and the resize); None
        without the file or when it holds no pair of integers in 1..4095."""
        p = os.path.join(self.seqs[i], "spacing.json")
        if not os.path.exists(p):
            return None
        try:
            with open(p) as f:
                return _spacing_pair(json.load(f).get("spacing_um"))
        except (ValueError, AttributeError):
            return None

    def native_spacing_um(self, i):
        """The sequence's native_spacing.json "spacing_um" [row_um, col_um] (tools/convert_camus.py --native-spacing: the NIfTI pixdim itself,
        the micrometres per pixel of the native frames); None without the file or when it holds no pair of integers in 1..4095."""
        p = os.path.join(self.seqs[i], "native_spacing.json")
        if not os.path.exists(p):
            return None
        try:
            with open(p) as f:
                return _spacing_pair(json.load(f).get("spacing_um"))
        except (ValueError, AttributeError):
            return None

    def _picked(self, i):
        """The frame files of sequence i that make its clip, in order (one pick for __getitem__ and native_target)"""
        fr = sorted(glob.glob(os.path.join(self.seqs[i], "frame_*.png")))
        if not fr:
            raise FileNotFoundError(f"{self.seqs[i]} holds no frame_*.png")
        pick = np.round(np.linspace(0, len(fr) - 1, self.T)).astype(int) if len(fr) >= self.T else \
            np.minimum(np.arange(self.T), len(fr) - 1)
        return fr, pick

    def native_hw(self, i) -> Optional[Tuple[int, int]]:
        """(h0, w0) of sequence i's native label frames (tools/convert_camus.py --native-masks: native_mask_XXX.png, all of one size), or None
        for a tree written without them."""
        nm = sorted(glob.glob(os.path.join(self.seqs[i], "native_mask_*.png")))
        if not nm:
            return None
        from PIL import Image
        with Image.open(nm[0]) as im:
            w0, h0 = im.size
        return int(h0), int(w0)

    def native_target(self, i) -> Optional[torch.Tensor]:
        """uint8 [T, h0, w0]: the labels of clip i's frames as the dataset stores them, untouched by any resize -- the same frame pick as
        __getitem__, IGNORE_LABEL on a frame without a native_mask file; None for a tree without native masks."""
        hw = self.native_hw(i)
        if hw is None:
            return None
        from PIL import Image
        fr, pick = self._picked(i)
        out = np.full((self.T,) + hw, IGNORE_LABEL, np.uint8)
        for t, j in enumerate(pick):
            p = os.path.join(os.path.dirname(fr[j]), os.path.basename(fr[j]).replace("frame_", "native_mask_"))
            if os.path.exists(p):
                m = np.asarray(Image.open(p), np.uint8)
                if m.shape != hw:
                    raise ValueError(f"{p}: {m.shape[0]} x {m.shape[1]} among native masks of {hw[0]} x {hw[1]}")
                out[t] = m
        return torch.from_numpy(out)

    def native_frames(self, i) -> Optional[torch.Tensor]:
        """uint8 [T, h0, w0]: the image frames of clip i at the sequence's own size (tools/convert_camus.py --native-frames:
        native_frame_XXX.png, grey, all of one size) -- the same frame pick as __getitem__; what ops.frames_from_native and predict.py take.
        None for a tree without them, or when a picked frame has no such file."""
        from PIL import Image
        fr, pick = self._picked(i)
        out = []
        for j in pick:
            p = os.path.join(os.path.dirname(fr[j]), "native_" + os.path.basename(fr[j]))
            if not os.path.exists(p):
                return None
            a = np.asarray(Image.open(p).convert("L"), np.uint8)
            if out and a.shape != out[0].shape:
                raise ValueError(f"{p}: {a.shape[0]} x {a.shape[1]} among native frames of {out[0].shape[0]} x {out[0].shape[1]}")
            out.append(a)
        return torch.from_numpy(np.stack(out))

    def __getitem__(self, i):
        from PIL import Image
        fr, pick = self._picked(i)
        xs, ys = [], []
        for j in pick:
            img = np.asarray(Image.open(fr[j]).convert("RGB"), np.uint8) if self.as_uint8 else np.asarray(Image.open(fr[j]).convert("RGB"), np.float32) / 255.0
            mk = fr[j].replace("frame_", "mask_")
            ldt = np.uint8 if self.as_uint8 else np.int64
            xs.append(img)
            ys.append(np.asarray(Image.open(mk), ldt) if os.path.exists(mk) else np.full(img.shape[:2], IGNORE_LABEL, ldt))
        return torch.from_numpy(np.stack(xs)).permute(0, 3, 1, 2).contiguous(), torch.from_numpy(np.stack(ys))


def clip_spacing_table(ds, cfg) -> Optional[torch.Tensor]:
    """int32 [len(ds), 2] (host) = every clip's (row_um, col_um): the dataset's own spacing_um(i), else cfg.data.spacing_um; None as soon as
    one clip has neither (then nothing is measured in mm: a table with holes would average over a different set of clips)."""
    fallback = _spacing_pair(cfg.data.spacing_um) if cfg.data.spacing_um is not None else None
    own = getattr(ds, "spacing_um", None)
    rows = []
    for i in range(len(ds)):
        sp = own(i) if own is not None else None
        sp = sp if sp is not None else fallback
        if sp is None:
            return None
        rows.append(sp)
    return torch.tensor(rows, dtype=torch.int32).reshape(len(rows), 2)


def native_spacing_table(ds, cfg) -> Optional[torch.Tensor]:
    """int32 [len(ds), 2] (host) = every clip's (row_um, col_um) per NATIVE pixel: the dataset's own native_spacing_um(i), else
    cfg.data.native_spacing_um; None as soon as one clip has neither (clip_spacing_table's rule, for the native frames)."""
    fallback = _spacing_pair(cfg.data.native_spacing_um) if cfg.data.native_spacing_um is not None else None
    own = getattr(ds, "native_spacing_um", None)
    rows = []
    for i in range(len(ds)):
        sp = own(i) if own is not None else None
        sp = sp if sp is not None else fallback
        if sp is None:
            return None
        rows.append(sp)
    return torch.tensor(rows, dtype=torch.int32).reshape(len(rows), 2)


NATIVE_MAX_SIDE = 2048


def native_target_table(ds) -> Optional[torch.Tensor]:
    """int32 [len(ds), 2] (host) = every clip's native (h0, w0), the size of its native_target(i); None as soon as one clip has none or a side
    outside 1..NATIVE_MAX_SIDE, and for a dataset without native_hw(i) (then nothing is evaluated at native resolution: a table with holes
    would average over a different set of clips)."""
    own = getattr(ds, "native_hw", None)
    if own is None or getattr(ds, "native_target", None) is None:
        return None
    rows = []
    for i in range(len(ds)):
        hw = own(i)
        if hw is None or not (1 <= hw[0] <= NATIVE_MAX_SIDE and 1 <= hw[1] <= NATIVE_MAX_SIDE):
            return None
        rows.append((int(hw[0]), int(hw[1])))
    return torch.tensor(rows, dtype=torch.int32).reshape(len(rows), 2)


def clip_length_table(ds) -> torch.Tensor:
    """int32 [len(ds)] (host) = every clip's number of valid frames for ops.lv_beats: the dataset's own length(i) where it has one, else its
    clip length `frames` (attribute T)."""
    own = getattr(ds, "length", None)
    return torch.tensor([int(own(i)) if own is not None else int(ds.T) for i in range(len(ds))], dtype=torch.int32).reshape(len(ds))


def view_pair_table(ds):
    """(pairs int32 [P, 2] (host) = the clip indices of the 2CH and of the 4CH view of every patient that has both, in the order the patients
    first appear; the number of patients with one of the two views only) for ops.lv_biplane; None for a dataset without patient(i) / view(i).
    A patient's first sequence of a view counts."""
    patient, view = getattr(ds, "patient", None), getattr(ds, "view", None)
    if patient is None or view is None:
        return None
    seen = {}
    for i in range(len(ds)):
        seen.setdefault(patient(i), {}).setdefault(view(i), i)
    rows = [(v["2CH"], v["4CH"]) for v in seen.values() if "2CH" in v and "4CH" in v]
    single = sum(1 for v in seen.values() if ("2CH" in v) != ("4CH" in v))
    return torch.tensor(rows, dtype=torch.int32).reshape(len(rows), 2), single


def build_dataset(cfg, split: str = "train", n_synthetic: int = 256, as_uint8: bool = False) -> Dataset:
    """as_uint8: frames as uint8 [T,3,H,W] (0..255: what the files hold) and labels as uint8 (IGNORE_LABEL = 255 fits) instead of float32 in
    [0,1] and int64 -- a fifth of the bytes per batch across PCIe (EchoNet shape, 16 clips: 26 MB instead of 128 MB); the entry points ask for
    it and scale on the GPU (gdkvm_amd.pipeline.DevicePrefetcher).  The HIP loss and mask kernels take uint8 labels as they are."""
    d = cfg.data
    if d.kind == "synthetic" or not cfg.data_path:
        return SyntheticEchoClips(n_synthetic if split == "train" else max(8, n_synthetic // 8), d.frames, d.size,
                                  d.num_classes, seed=cfg.seed + (0 if split == "train" else 7919), as_uint8=as_uint8, beats=d.synthetic_beats)
    if d.kind == "npy_clips":
        return NpzClips(cfg.data_path, split, d.frames, as_uint8=as_uint8)
    if d.kind == "echonet_npz":
        return EchoNetNpz(cfg.data_path, split, d.frames, as_uint8=as_uint8, whole=d.whole_video)
    if d.kind == "camus_png":
        return CamusPng(cfg.data_path, split, d.frames, as_uint8=as_uint8)
    raise ValueError(f"unknown data.kind {d.kind!r}")
