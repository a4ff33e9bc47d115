"""Native clips in, native masks and LV figures out: the public entry for frames as a scanner or a dataset hands them over.

segment_native(model, cfg, clips, spacing_um=None) takes a list of uint8 [T, h0, w0] grey clips (one T per call, every clip its own frame
size) through
    1. ops.pack_native and one host-to-device copy of the ragged bytes,
    2. ops.frames_from_native: the exact-integer area average onto the config's grid (data.size x data.size), three equal planes, in the
       model's dtype (the bytes a tree written by tools/convert_camus.py --resample area holds, cast as the DevicePrefetcher casts them),
    3. the forward as eval.py runs it (pipeline.SegmentRunner; GDKVM_FWD_GRAPH / GDKVM_FWD_IN_FLIGHT as there),
    4. the configured post-processing in eval.py's order and with its keys: data.temporal_vote, data.lv_keep_largest, data.lv_fill_holes
       (data.lv_fill_max_area),
    5. ops.mask_to_native of the post-processed mask: every clip's masks at its own frame size,
and, with data.lv_class >= 0, measures the class on the grid per clip: ops.lv_measure / lv_ef (pixel^3; EF is a ratio), ops.lv_beats with
data.lv_beats, and with a native pixel spacing (row_um, col_um) ops.lv_measure_mm at the grid spacing (rint(row_um h0 / H),
rint(col_um w0 / W)) -- tools/convert_camus.py's spacing_um formula; the mL keys are left out, with the reason, when that falls outside
1..4095.  With data.native_lv an `lv_native` entry per clip holds the same class measured on the NATIVE post-processed masks of step 5
(ops.lv_measure_native / lv_ef: ed_frame, es_frame, valid_frames, ef, and with a native spacing -- each component rint-ed to integer um and
recorded -- edv_ml and esv_ml; a clip without a usable spacing is measured at 1 x 1 um and reports the EF, with the reason under
lv_native_ml_omitted).  With data.lv_strain a `strain` entry per clip holds the global longitudinal strain of the class's endocardial contour between
those ED / ES frames, the peak strain and its frame, and the contour and apex-to-annulus lengths at ED and ES (ops.lv_contour /
contour_lengths / lv_strain; mm for a clip with a grid spacing, else px).  With overlay=True it also draws what a person looks at, ops.overlay_native of the native frames under those native masks (the
configuration's `overlay:` section); overlay_clip draws one clip with an optional reference mask, which is what eval.py's
eval_stage.vis_overlay writes.  Everything after the copy runs on the device: there is no CPU path for the forward, and a CPU model is
refused.  ops.surface_distance_native, the native family's measurement against a tracing, has no place here: a prediction has no target
(eval.py reports it as native.surface).

load_input reads what predict.py's command line names: a .npy file ([T, h0, w0] uint8), a .npz file (`frames`, optional `spacing_um` =
the NATIVE micrometres per pixel) or a directory of native_frame_*.png (else frame_*.png), where a spacing.json with "native_hw" (the
converter's: the spacing of the RESIZED grid) is rescaled back to native micrometres by the size of the directory's frame_*.png."""
from __future__ import annotations

import glob
import json
import os
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .config import beat_prominence_permille


def grid_spacing_um(spacing_um, h0: int, w0: int, H: int, W: int) -> Optional[Tuple[int, int]]:
    """The grid's (row_um, col_um) of a native h0 x w0 frame with pixels of spacing_um = (row_um, col_um) taken to H x W: rint(row_um h0 / H),
    rint(col_um w0 / W), tools/convert_camus.py's formula; None when a value is not finite or a result falls outside 1..SPACING_UM_MAX."""
    try:
        r, c = float(spacing_um[0]), float(spacing_um[1])
    except (TypeError, ValueError, IndexError):
        return None
    if not (np.isfinite(r) and np.isfinite(c)):
        return None
    row, col = float(np.rint(r * h0 / H)), float(np.rint(c * w0 / W))
    if not (1 <= row <= ops.SPACING_UM_MAX and 1 <= col <= ops.SPACING_UM_MAX):
        return None
    return int(row), int(col)


def native_spacing_um(spacing_um) -> Optional[Tuple[int, int]]:
    """The native pixel's (row_um, col_um) as the integers ops.lv_measure_native takes: each component rint-ed; None when a value is not
    finite or a result falls outside 1..SPACING_UM_MAX."""
    return grid_spacing_um(spacing_um, 1, 1, 1, 1)


def make_runner(model):
    """pipeline.SegmentRunner with eval.py's environment switches; one per model, kept over the calls so that repeated batch shapes are captured"""
    from .pipeline import SegmentRunner
    return SegmentRunner(model, graph=os.environ.get("GDKVM_FWD_GRAPH", "1") != "0", in_flight=int(os.environ.get("GDKVM_FWD_IN_FLIGHT", "2")))


def _overlay_args(cfg) -> dict:
    """The `overlay:` section of the configuration as ops.overlay_native's keyword arguments"""
    o = cfg.overlay
    return dict(width=o.width, alpha=o.alpha, palette=o.palette, reference_palette=o.reference_palette)


def overlay_clip(frames_u8: torch.Tensor, mask: torch.Tensor, cfg, reference: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One clip's overlay pictures, uint8 [T, h, w, 3] on the mask's device: frames_u8 [T, h, w] uint8 grey frames, mask [T, h, w] uint8
    labels and optionally a reference mask of that shape whose contour is drawn too (eval.py: the target), through ops.overlay_native with the
    configuration's `overlay:` section and data.num_classes.  frames_u8 and reference may live on the host: they are copied to the mask's
    device."""
    if not all(isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.dim() == 3 for t in (frames_u8, mask)) \
            or frames_u8.shape != mask.shape or (reference is not None and (not isinstance(reference, torch.Tensor) or reference.dtype != torch.uint8
                                                                            or reference.shape != mask.shape)):
        raise ops.GdkvmError("overlay_clip: frames_u8, mask and reference must be uint8 [T, h, w] tensors of one shape")
    T, h, w = (int(n) for n in mask.shape)
    dev = mask.device
    flat = lambda t: t.to(dev).contiguous().reshape(-1)
    rgb = ops.overlay_native(flat(frames_u8), flat(mask), [(h, w)], T, cfg.data.num_classes,
                             reference=None if reference is None else flat(reference), **_overlay_args(cfg))
    return ops.native_rgb_frames(rgb, [(h, w)], T, 0)


def segment_native(model, cfg, clips: Sequence[torch.Tensor], spacing_um=None, runner=None, overlay: bool = False) -> dict:
    """See the module's head.  clips: uint8 [T, h0, w0] tensors with one T (host or device); spacing_um: None or, per clip, None or the native
    (row_um, col_um); runner: make_runner(model) kept by the caller over several calls (None: one is made for this call).  Returns
    {"masks": [uint8 [T, h0, w0] per clip, on the model's device], "grid_mask": uint8 [clips, T, H, W] (post-processed), "frames": the
    network's input [clips, T, 3, H, W], "sizes": [(h0, w0), ...], "report": {"clips", "frames", "grid", "forward", "per_clip": [...]}}.
    overlay=True keeps the device copy of the packed native bytes and adds "overlay": [uint8 [T, h0, w0, 3] per clip], ops.overlay_native of
    the native frames and the post-processed native masks with the configuration's `overlay:` section (no reference)."""
    clips = list(clips)
    flat, sizes = ops.pack_native([c.cpu() if isinstance(c, torch.Tensor) and c.is_cuda else c for c in clips])
    T = int(clips[0].shape[0])
    B = len(sizes)
    if spacing_um is not None and len(spacing_um) != B:
        raise ops.GdkvmError(f"segment_native: {len(spacing_um)} spacings for {B} clips")
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise ops.GdkvmError("segment_native: the model must be on a HIP device (the forward has no CPU path)")
    d = cfg.data
    H = W = int(d.size)
    ncls, lv_cls = d.num_classes, d.lv_class
    fdt = torch.bfloat16 if cfg.precision == "bf16" else torch.float32
    flat_dev = flat.to(dev)
    frames, _ = ops.frames_from_native(flat_dev, sizes, T, grid=(H, W), channels=3, dtype=fdt)
    if runner is None:
        runner = make_runner(model)
    mask, _ = runner(frames, None)
    measured = mask
    vote = d.temporal_vote
    keep = d.lv_keep_largest if lv_cls >= 0 else 0
    fillc = d.lv_fill_holes if lv_cls >= 0 else 0
    post = {}
    if vote:
        measured, tv, _ = ops.temporal_vote(measured, ncls, vote)
        post["temporal_vote"] = tv
    if keep:
        measured, lc = ops.largest_component(measured, cls=lv_cls, connectivity=keep, fill=0)
        post["largest_component"] = lc
    if fillc:
        measured, fh = ops.fill_holes(measured, cls=lv_cls, connectivity=fillc, max_area=d.lv_fill_max_area)
        post["fill_holes"] = fh
    native, _, _ = ops.mask_to_native(measured, sizes, ncls, want_out=True)
    masks = [ops.native_frames(native, sizes, T, b) for b in range(B)]
    pictures = None
    if overlay:
        rgb = ops.overlay_native(flat_dev, native, sizes, T, ncls, **_overlay_args(cfg))
        pictures = [ops.native_rgb_frames(rgb, sizes, T, b) for b in range(B)]
    r5 = lambda v: round(float(v), 5)
    per_clip = [{"native_hw": [h0, w0]} for h0, w0 in sizes]
    if vote:
        for b, row in enumerate(post["temporal_vote"][..., 0].sum(-1).tolist()):
            per_clip[b]["temporal_vote"] = {"radius": vote, "pixels_changed": int(row)}
    if keep:
        rem = (post["largest_component"][..., 1] - post["largest_component"][..., 2]).sum(-1).tolist()
        for b, row in enumerate(rem):
            per_clip[b]["largest_component"] = {"connectivity": keep, "pixels_removed": int(row)}
    if fillc:
        for b, row in enumerate(post["fill_holes"][..., 3].sum(-1).tolist()):
            per_clip[b]["fill_holes"] = {"connectivity": fillc, "max_area": d.lv_fill_max_area, "pixels_filled": int(row)}
    if lv_cls >= 0:
        p_stats, _, p_geom = ops.lv_measure(measured, cls=lv_cls)
        area, vol = p_stats[..., 0].contiguous(), p_geom[..., 1].contiguous()
        idx, val = ops.lv_ef(vol, area)
        for b, (i3, v3) in enumerate(zip(idx.tolist(), val.tolist())):
            per_clip[b]["lv"] = {"ed_frame": i3[0], "es_frame": i3[1], "valid_frames": i3[2], "edv_px3": r5(v3[0]), "esv_px3": r5(v3[1]),
                                 "ef": r5(v3[2])}
        q_vol = None
        if spacing_um is not None:
            grid_sp = [None if s is None else grid_spacing_um(s, h0, w0, H, W) for s, (h0, w0) in zip(spacing_um, sizes)]
            if any(g is not None for g in grid_sp):
                # a clip without a usable spacing is measured at 1 x 1 um and its mL keys are left out
                sp = torch.tensor([g or (1, 1) for g in grid_sp], dtype=torch.int32).reshape(B, 1, 2).to(dev)
                q_stats, _, q_geom = ops.lv_measure_mm(measured, sp, cls=lv_cls)
                q_vol = q_geom[..., 1].contiguous()
                m_picks, m_val = ops.lv_ef(q_vol, q_stats[..., 0].contiguous())
                m_idx, m_val = m_picks.tolist(), m_val.tolist()
            for b, g in enumerate(grid_sp):
                if g is not None:
                    per_clip[b]["lv_mm"] = {"grid_spacing_um": list(g), "ed_frame": m_idx[b][0], "es_frame": m_idx[b][1],
                                            "edv_ml": r5(m_val[b][0]), "esv_ml": r5(m_val[b][1]), "ef": r5(m_val[b][2])}
                else:
                    why = "no spacing" if spacing_um[b] is None else \
                        f"the grid spacing of {spacing_um[b][0]} x {spacing_um[b][1]} um pixels falls outside 1..{ops.SPACING_UM_MAX} um"
                    per_clip[b]["lv_mm_omitted"] = why
        if d.native_lv:
            # the same class on the native post-processed masks above, at every clip's own size with the spacing of the native pixel (each
            # component rint-ed to integer um); a clip without a usable spacing is measured at 1 x 1 um: its EF is a ratio, its mL keys are left out
            nat_sp = [None if s is None else native_spacing_um(s) for s in (spacing_um if spacing_um is not None else [None] * B)]
            n_stats, _, n_geom = ops.lv_measure_native(native, sizes, T, [s or (1, 1) for s in nat_sp], cls=lv_cls)
            n_idx, n_val = ops.lv_ef(n_geom[..., 1].contiguous(), n_stats[..., 0].contiguous())
            for b, (i3, v3) in enumerate(zip(n_idx.tolist(), n_val.tolist())):
                per_clip[b]["lv_native"] = {"ed_frame": i3[0], "es_frame": i3[1], "valid_frames": i3[2], "ef": r5(v3[2])}
                if nat_sp[b] is not None:
                    per_clip[b]["lv_native"].update(spacing_um=list(nat_sp[b]), edv_ml=r5(v3[0]), esv_ml=r5(v3[1]))
                else:
                    per_clip[b]["lv_native_ml_omitted"] = "no spacing" if spacing_um is None or spacing_um[b] is None else \
                        f"the native spacing of {spacing_um[b][0]} x {spacing_um[b][1]} um falls outside 1..{ops.SPACING_UM_MAX} um"
        if d.lv_beats:
            if q_vol is not None and all(g is not None for g in grid_sp):
                b_vol, unit = q_vol, "ml"
            else:
                b_vol, unit = vol, "px3"
            _, _, b_info, b_summ = ops.lv_beats(area, b_vol, None, distance=d.beat_distance, prominence_permille=beat_prominence_permille(cfg))
            for b, (bi, bs) in enumerate(zip(b_info.tolist(), b_summ.tolist())):
                per_clip[b]["beats"] = {"volume_unit": unit, "beats": bi[0], "end_systoles": bi[1], "frames_below_min": bi[2],
                                        "ef_mean": r5(bs[0]), "ef_min": r5(bs[1]), "ef_max": r5(bs[2]), "mean_cycle_frames": r5(bs[3])}
        if d.lv_strain:
            # the contour of the same post-processed mask: in mm at the lv_mm block's ED / ES for a clip with a grid spacing, else in pixels
            # at the lv block's
            c_args = dict(cls=lv_cls, wall=d.lv_wall_classes, base=d.lv_base_classes)
            forms = {"px": (ops.lv_contour(measured, **c_args), None, idx)}
            if q_vol is not None:
                forms["mm"] = (ops.lv_contour(measured, spacing_um=sp, **c_args), sp, m_picks)
            rows = {}
            for unit, (rec, usp, picks) in forms.items():
                lens = ops.contour_lengths(rec, usp)
                npx = rec[..., 0].contiguous()
                _, gp, pf, ok = ops.lv_strain(lens[..., 0].contiguous(), npx, picks)
                _, ga, _, oka = ops.lv_strain(lens[..., 2].contiguous(), npx, picks)
                rows[unit] = [t.tolist() for t in (lens, gp, pf, ok, ga, oka, picks)]
            for b in range(B):
                unit = "mm" if "mm" in rows and grid_sp[b] is not None else "px"
                lens, gp, pf, ok, ga, oka, picks = (r[b] for r in rows[unit])
                ed, es = picks[0], picks[1]
                at = lambda t, k: r5(lens[t][k]) if t >= 0 else 0.0
                per_clip[b]["strain"] = {"unit": unit, "ok": bool(ok), "gls": r5(gp[0]), "peak_strain": r5(gp[1]), "peak_frame": pf,
                                         "wall_ed": at(ed, 0), "wall_es": at(es, 0), "landmarks": bool(oka), "axis_ed": at(ed, 2),
                                         "axis_es": at(es, 2), "axis_shortening": r5(ga[0])}
    report = {"clips": B, "frames": T, "grid": [H, W], "forward": {"graph_replays": runner.replays, "eager_calls": runner.eager_calls},
              "per_clip": per_clip}
    res = {"masks": masks, "grid_mask": measured, "frames": frames, "sizes": sizes, "report": report}
    if overlay:
        res["overlay"] = pictures
    return res


def _grey(path: str) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("L"), np.uint8)


def load_input(path: str):
    """(name, frames uint8 [T, h0, w0] tensor, native spacing (row_um, col_um) or None) of one command-line input (the module's head)"""
    name = os.path.basename(os.path.normpath(path))
    spacing = None
    if os.path.isdir(path):
        files = sorted(glob.glob(os.path.join(path, "native_frame_*.png"))) or sorted(glob.glob(os.path.join(path, "frame_*.png")))
        if not files:
            raise ValueError(f"{path}: holds neither native_frame_*.png nor frame_*.png")
        fr = [_grey(p) for p in files]
        if any(a.shape != fr[0].shape for a in fr):
            raise ValueError(f"{path}: frames of different sizes")
        arr = np.stack(fr)
        sj = os.path.join(path, "spacing.json")
        resized = sorted(glob.glob(os.path.join(path, "frame_*.png")))
        if os.path.exists(sj) and resized:
            try:
                with open(sj) as f:
                    meta = json.load(f)
                sp, hw = meta.get("spacing_um"), meta.get("native_hw")
                gh, gw = _grey(resized[0]).shape
                if sp and hw and [int(hw[0]), int(hw[1])] == list(arr.shape[1:]):
                    # spacing.json holds the RESIZED grid's spacing: back to the native pixel by the inverse of the converter's formula
                    spacing = (float(sp[0]) * gh / arr.shape[1], float(sp[1]) * gw / arr.shape[2])
                elif sp and list(arr.shape[1:]) == [gh, gw]:
                    spacing = (float(sp[0]), float(sp[1]))         # the frames ARE the resized ones: the spacing is theirs
            except (ValueError, TypeError, AttributeError, IndexError):
                spacing = None
    elif path.endswith(".npz"):
        name = name[:-4]
        with np.load(path) as z:
            if "frames" not in z.files:
                raise ValueError(f"{path}: no `frames` array")
            arr = z["frames"]
            if "spacing_um" in z.files and np.asarray(z["spacing_um"]).size == 2:
                s = np.asarray(z["spacing_um"], np.float64).reshape(2)
                spacing = (float(s[0]), float(s[1]))
    elif path.endswith(".npy"):
        name = name[:-4]
        arr = np.load(path)
    else:
        raise ValueError(f"{path}: neither a .npy / .npz file nor a directory of PNG frames")
    if arr.ndim != 3 or arr.dtype != np.uint8 or arr.shape[0] < 1:
        raise ValueError(f"{path}: frames must be uint8 [T, h0, w0], got {arr.dtype} {arr.shape}")
    return name, torch.from_numpy(np.ascontiguousarray(arr)), spacing


def build_model(cfg, weights: str = "", ema: bool = False, dev=None):
    """The model as eval.py builds and loads it: GDKVMConfig from the run configuration, the checkpoint's "model" (or "ema") entry, folded for
    inference, in the configuration's precision, channels_last, on `dev`."""
    from .model import GDKVM, GDKVMConfig
    mcfg = GDKVMConfig(num_classes=cfg.data.num_classes, heads=cfg.model.heads, key_dim=cfg.model.key_dim,
                       value_dim=cfg.model.value_dim, rule=cfg.model.rule,
                       scan_segments=cfg.model.scan_segments, mask_feedback=cfg.model.mask_feedback)
    model = GDKVM(mcfg).eval()
    if ema and not weights:
        raise SystemExit("predict.py: --ema needs --weights (the averaged weights live in a checkpoint)")
    if weights:
        ck = torch.load(weights, map_location="cpu")
        if ema and "ema" not in ck:
            raise SystemExit(f"predict.py: --ema: {weights} holds no averaged weights (no \"ema\" entry): it was trained without "
                             "optim.kind=native and optim.ema_decay > 0")
        model.load_state_dict(ck["ema"] if ema else ck["model"])
    model = model.fuse_for_inference().to(dev)
    if cfg.precision == "bf16":
        model = model.to(torch.bfloat16)
    return model.to(memory_format=torch.channels_last)


def main(argv=None) -> dict:
    import argparse
    from .config import load_config
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser(description="native clips in, native masks and report.json out")
    ap.add_argument("--config", default=os.path.join(root, "config", "config_gdkvm_01.yaml"))
    ap.add_argument("--weights", default="")
    ap.add_argument("--ema", action="store_true", help="use the checkpoint's EMA weights (optim.ema_decay > 0 runs)")
    ap.add_argument("--out", required=True, help="directory for <name>/mask_XXX.png and report.json")
    ap.add_argument("--overlay", action="store_true",
                    help="also write <name>/overlay_XXX.png: the frame in grey, the predicted classes tinted, their contours opaque "
                         "(the configuration's overlay: section)")
    ap.add_argument("inputs", nargs="+", metavar="INPUT|key=value",
                    help=".npy / .npz clips or directories of PNG frames; arguments of the form key=value that name no file override the configuration")
    args = ap.parse_args(argv)
    inputs = [a for a in args.inputs if os.path.exists(a) or "=" not in a]
    overrides = [a for a in args.inputs if a not in inputs]
    if not inputs:
        raise SystemExit("predict.py: no input")
    cfg = load_config(args.config, overrides)
    ops.require_native()
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(cfg.seed)
    model = build_model(cfg, args.weights, args.ema, dev)
    runner = make_runner(model)
    from PIL import Image
    loaded, seen = [], {}
    for p in inputs:
        name, fr, sp = load_input(p)
        seen[name] = seen.get(name, 0) + 1
        loaded.append((name if seen[name] == 1 else f"{name}_{seen[name]}", p, fr, sp))
    by_T = {}
    for k, item in enumerate(loaded):
        by_T.setdefault(int(item[2].shape[0]), []).append(k)
    entries = [None] * len(loaded)
    os.makedirs(args.out, exist_ok=True)
    for T, ks in by_T.items():
        for lo in range(0, len(ks), max(1, cfg.batch_size)):
            part = ks[lo:lo + max(1, cfg.batch_size)]
            res = segment_native(model, cfg, [loaded[k][2] for k in part], [loaded[k][3] for k in part], runner=runner, overlay=args.overlay)
            for j, (k, m, rep) in enumerate(zip(part, res["masks"], res["report"]["per_clip"])):
                name = loaded[k][0]
                os.makedirs(os.path.join(args.out, name), exist_ok=True)
                for t, fr in enumerate(m.cpu().numpy()):
                    Image.fromarray(fr).save(os.path.join(args.out, name, f"mask_{t:03d}.png"))
                if args.overlay:
                    for t, fr in enumerate(res["overlay"][j].cpu().numpy()):
                        Image.fromarray(fr).save(os.path.join(args.out, name, f"overlay_{t:03d}.png"))
                entries[k] = {"name": name, "input": loaded[k][1], "frames": T, **rep}
    report = {"clips": len(loaded), "grid": [cfg.data.size, cfg.data.size], "weights": args.weights, "ema": bool(args.ema),
              "forward": {"graph_replays": runner.replays, "eager_calls": runner.eager_calls}, "per_clip": entries}
    with open(os.path.join(args.out, "report.json"), "w") as f:
        json.dump(report, f)
    print(json.dumps(report), flush=True)
    return report
