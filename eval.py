#!/usr/bin/env python3
"""Evaluation entry point: per-class Dice / IoU of the argmax masks over a dataset split and, for class `data.lv_class`, the left-ventricular
volumes and ejection fraction measured from the masks on the device (ops.lv_measure / lv_ef: pixel^3 of the network's input grid, isotropic
pixels assumed; EF is a ratio); clips sharded over the GPUs of one node (no data-path collective; only the integer Dice counts and the eight
EF sums are summed at the end).  With `data.lv_keep_largest` = 4 or 8 the PREDICTED mask is measured after ops.largest_component kept the
largest 4- / 8-connected component of that class (fill 0; the target is a tracing and is measured as it is): the `lv` block is then the
post-processed one, a `largest_component` block reports what was removed and the class's Dice / IoU after it, and every other key is still
computed from the unfiltered mask.  With `data.surface_class` >= 0 a `surface` block reports the class's mean Hausdorff distance, HD95 and
ASSD between predicted mask and target (ops.surface_distance / surface_metrics: pixels of the input grid, over the labelled frames where both
have a surface).  The surface distances are those of the unfiltered mask, whatever `data.lv_keep_largest` says.  With `data.lv_fill_holes`
= 4 or 8 (the connectivity of the class's COMPLEMENT) ops.fill_holes then fills the holes of that class in the predicted mask -- after the
largest-component filter when that is on too, so that the islands' holes never matter; `data.lv_fill_max_area` > 0 fills only the holes of at
most that many pixels -- and the `lv` block is that of the filled mask; a `fill_holes` block reports the holes, the pixels filled and the
class's Dice / IoU after it, and every other key, the `largest_component` and `surface` blocks included, is computed as before.  With
`data.temporal_vote` = r in 1..7 ops.temporal_vote first smooths the predicted masks of every clip over time (each pixel takes the class most
of the frames t - r .. t + r have there), so that the unlabelled frames of a clip steady the labelled ones: the voted mask is what enters the
largest-component filter, the hole filling and the `lv` block, the `largest_component` block's Dice / IoU start from the vote's counts, and a
`temporal_vote` block reports the frames and pixels changed, the pixels per frame that differ from the previous frame before and after the
vote (temporal instability) and the voted mask's Dice; `dice_per_class`, `iou_per_class` and the `surface` block are still those of the
unfiltered mask.

With a pixel spacing for every clip (gdkvm_amd.data.clip_spacing_table: the dataset's own, e.g. the spacing.json beside a CAMUS sequence, else
`data.spacing_um` = [row_um, col_um]) the same masks are measured a second time in physical units: an `lv_mm` block (with `lv_class` >= 0) holds
the EF statistics computed from the volumes in mL (ops.lv_measure_mm: the long axis is found in the physical plane, and ED / ES are the target's
frames picked on its mL curve) and the mean absolute error and bias of EDV and ESV in mL; a `surface_mm` block (with `surface_class` >= 0)
holds the mean HD, HD95 and ASSD in mm (ops.surface_distance_mm / surface_metrics_mm).  Every other key keeps its value; without a spacing for
every clip neither block appears and nothing new runs.

With `data.lv_beats` (and `lv_class` >= 0) the clip is also read beat by beat (ops.lv_beats on the area curve of the post-processed predicted
masks and on their volume curve, mL with a spacing, else pixel^3; `data.beat_distance`, `data.beat_prominence`; only the frames a clip's
dataset calls its own count, gdkvm_amd.data.clip_length_table): a `beats` block holds `clips`, `beats_per_clip` and `mean_cycle_frames` over
the clips whose class never vanished, `clips_dropped_below_min` (those where it did: a vanished class is a false systole), and, against the
target's own curves where the target labels every valid frame of a clip, `clips_with_target`, `ef_mae`, `ef_bias`, `ef_pearson_r` of the mean
beat EF and `systole_count_agreement`; where the dataset knows an EF per file (EchoNetNpz.file_ef), the same EF statistics against it as
`vs_file_ef`.  Every other key keeps its value; the `lv` block's one ED / ES / EF per clip is right for clips of one beat only.

With `data.lv_biplane` (and `lv_class` >= 0, a spacing for every clip and a dataset that names every clip's patient and view: camus_png) the
2CH and the 4CH clip of a patient are combined into ONE volume per frame by the bi-plane method of disks (ops.lv_biplane on the records
ops.lv_measure_mm left of the post-processed prediction and of the target, kept for the whole split in device tables and summed over the ranks:
a pair may straddle batches and shards) -- the quantity CAMUS states per patient.  A `biplane` block, behind every other key, holds `pairs`,
`patients_single_view`, `pairs_with_target` (the target's bi-plane curve has two frames and an EDV; ED / ES are picked on it and the
prediction is read there), the EF statistics of prediction against target, `edv_mae_ml`, `edv_bias_ml`, `esv_mae_ml`, `esv_bias_ml`,
`length_mismatch_mean` and `pairs_length_mismatch_over_10pct` (how far the prediction's two long axes are apart at ED, as a fraction of the
longer) and, where the dataset knows what the files state (CamusPng.info: the 2CH view's value, else the 4CH view's), a `vs_file` block:
`pairs_with_ef`, EF MAE / bias / r of the prediction against the file, `target_ef_mae` (how well this method on the tracings reproduces the
file) and the same for EDV and ESV in mL.  Disk j of both views must count from the same end of the ventricle: both views apex up, as CAMUS
stores them.  Every other key keeps its value.

With `data.native_eval` (and a dataset that has a native target for every clip, gdkvm_amd.data.native_target_table: camus_png trees written by
tools/convert_camus.py --native-masks, npy_clips with a `native_target` array) the predicted masks are also compared with the tracing as the
dataset stores it, at every clip's OWN frame size -- the Dice a published figure is computed with, which the keys above, measured on the
network's grid against a nearest-neighbour down-sampled tracing, are not.  ops.mask_to_native takes the raw predicted mask to the native size
(half-pixel-centre bilinear on the one-hot planes, exact integers) and counts it against the native target in the same pass; a frame counts
when its native target has a pixel of some class.  A `native` block holds `dice_per_class`, `mean_foreground_dice`, `iou_per_class`,
`mean_foreground_iou` (the grid's formulas and rounding), `pixels` (the native pixels compared) and `frames`; with any of `temporal_vote`,
`lv_keep_largest`, `lv_fill_holes` on, `native.post` holds the same keys for the post-processed mask.  With `data.native_surface_class` >= 0
(which needs `native_eval`) the RAW predicted mask at native size (ops.mask_to_native's out) is also measured against the native target with
ops.surface_distance_native, and a `native.surface` block holds `class`, `unit`, `frames`, `frames_one_empty`, `hd_mean`, `hd95_mean`,
`assd_mean` over the frames that count above (surface_metrics_mm / surface_summary, rounded like `surface_mm`): in mm (`unit`: "mm") with
the spacing of the NATIVE pixel for every clip (gdkvm_amd.data.native_spacing_table: the dataset's own, e.g. the native_spacing.json of
tools/convert_camus.py --native-spacing, else `data.native_spacing_um`), else in native pixels (`unit`: "px", measured at 1000 x 1000 um so
that one pixel reads as 1.0).  Like the grid's `surface` block these are the distances of the unfiltered mask.  With `data.native_lv`
(which needs `native_eval` and `lv_class` >= 0) the volumes are measured there too: ops.lv_measure_native on the POST-PROCESSED predicted
mask at native size (the raw one when no post-processing is on) and on the native target, ED / ES picked on the target's curve with
ops.lv_ef as for `lv_mm`, and a `native.lv` block holds the `lv_mm` keys (EF statistics, EDV / ESV `_mae_ml` / `_bias_ml`), `unit`: "mL" and
`frames` with a native spacing for every clip, else the EF statistics, `unit`: "px3" (measured at 1000 x 1000 um) and `frames`.  Every
other key keeps its value; with the keys off nothing new runs.

With `data.lv_strain` (and `lv_class` >= 0) the contour of the class is measured as well (ops.lv_contour on the post-processed prediction and on
the target: its border with `data.lv_wall_classes` is the endocardium, its border with `data.lv_base_classes` the mitral plane): a `strain`
block holds the `unit` of the lengths ("mm" with a spacing for every clip, and then ED / ES are the `lv_mm` block's frames, else "px" and the
`lv` block's frames), `clips_with_strain`, `gls_mae`, `gls_bias`, `gls_pearson_r`, `mean_ref_gls`, `mean_pred_gls` of the global longitudinal
strain (L_ES - L_ED) / L_ED of the endocardial contour (ops.contour_lengths / lv_strain), and a `long_axis` block with the same statistics of
the apex-to-annulus shortening over the clips whose ED and ES frames have a base interface on both sides, and `clips_without_landmarks`.
With an empty `lv_base_classes` (a binary dataset: `lv_wall_classes: [0]`) the strain is that of the whole outline and there are no
landmarks; the block says so.  Every other key keeps its value; with the key off nothing new runs.

--ema evaluates the checkpoint's averaged weights (its "ema" entry, written by runs with optim.ema_decay > 0) instead of the trained ones.

    python eval.py --config config/config_gdkvm_01.yaml --weights outputs/gdkvm_step3000.pth [--ema] [key=value ...]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(ROOT, "config", "config_gdkvm_01.yaml"))
    ap.add_argument("--weights", default="")
    ap.add_argument("--split", default="val")
    ap.add_argument("--ema", action="store_true", help="evaluate the checkpoint's EMA weights (optim.ema_decay > 0 runs)")
    ap.add_argument("overrides", nargs="*")
    args = ap.parse_args(argv)

    from gdkvm_amd import ops
    from gdkvm_amd.config import beat_prominence_permille, load_config
    from gdkvm_amd.data import build_dataset, clip_length_table, clip_spacing_table, native_spacing_table, native_target_table, view_pair_table
    from gdkvm_amd.distributed import init_from_env, shard_range
    from gdkvm_amd.model import GDKVM, GDKVMConfig

    cfg = load_config(args.config, args.overrides)
    ops.require_native()
    rank, world, local = init_from_env()
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    torch.manual_seed(cfg.seed)
    mcfg = GDKVMConfig(num_classes=cfg.data.num_classes, heads=cfg.model.heads, key_dim=cfg.model.key_dim,
                       value_dim=cfg.model.value_dim, rule=cfg.model.rule,
                       scan_segments=cfg.model.scan_segments, mask_feedback=cfg.model.mask_feedback)
    model = GDKVM(mcfg).eval()
    if args.ema and not args.weights:
        raise SystemExit("eval.py: --ema needs --weights (the averaged weights live in a checkpoint)")
    if args.weights:
        ck = torch.load(args.weights, map_location="cpu")
        if args.ema and "ema" not in ck:
            raise SystemExit(f"eval.py: --ema: {args.weights} holds no averaged weights (no \"ema\" entry): it was trained without "
                             "optim.kind=native and optim.ema_decay > 0")
        model.load_state_dict(ck["ema"] if args.ema else ck["model"])
    model = model.fuse_for_inference().to(dev)
    if cfg.precision == "bf16":
        model = model.to(torch.bfloat16)
    model = model.to(memory_format=torch.channels_last)

    from gdkvm_amd.pipeline import DevicePrefetcher, SegmentRunner
    ds = build_dataset(cfg, args.split, as_uint8=True)            # bytes across PCIe; cast and scaled on the GPU
    lo, hi = shard_range(len(ds), world, rank)
    spacing = clip_spacing_table(ds, cfg)                         # int32 [clips, 2] micrometres per pixel, or None: no mL / mm blocks
    if spacing is not None:
        if int(spacing.min()) < 1 or int(spacing.max()) > ops.SPACING_UM_MAX:
            raise SystemExit(f"eval.py: a pixel spacing outside 1..{ops.SPACING_UM_MAX} micrometres")
        spacing = spacing.to(dev)
    counts = torch.zeros(cfg.data.num_classes, 3, dtype=torch.int64, device=dev)
    lv_cls = cfg.data.lv_class
    mm = spacing is not None
    # ops.ef_summary, accumulated on the device and read once at the end; with a spacing, behind it the same eight sums of the EF, the EDV and
    # the ESV measured in mL
    ef_sums = torch.zeros(8 + (24 if mm else 0), dtype=torch.float64, device=dev)
    keep = cfg.data.lv_keep_largest if lv_cls >= 0 else 0         # 0 = off: no new call below
    # the filtered mask's counts [ncls, 3], then frames changed and pixels removed: accumulated on the device, read once at the end
    lc_acc = torch.zeros(cfg.data.num_classes * 3 + 2, dtype=torch.int64, device=dev) if keep else None
    fillc = cfg.data.lv_fill_holes if lv_cls >= 0 else 0          # 0 = off: no new call below
    # the filled mask's counts of lv_class [3], then frames changed, holes and pixels filled: accumulated on the device, read once at the end
    fh_acc = torch.zeros(6, dtype=torch.int64, device=dev) if fillc else None
    vote = cfg.data.temporal_vote                                 # 0 = off: no new call below
    # ops.vote_summary: the voted mask's counts [ncls, 3], then pixels changed, frames changed, flips before, flips after, frames
    tv_acc = torch.zeros(cfg.data.num_classes * 3 + 5, dtype=torch.int64, device=dev) if vote else None
    s_cls = cfg.data.surface_class                                # -1 = off: no new call below
    # ops.surface_summary, accumulated on the device; with a spacing, behind it the same five sums in mm
    sd_sums = torch.zeros(5 + (5 if mm else 0), dtype=torch.float64, device=dev) if s_cls >= 0 else None
    beats_on = cfg.data.lv_beats and lv_cls >= 0                  # off: no new call below
    if beats_on:
        # clips, dropped, kept, their beats, clips with a cycle, the cycles; ops.beats_summary against the target [11]; ops.ef_summary against
        # the files' EF [8]: accumulated on the device, read once at the end
        bt_acc = torch.zeros(6 + 11 + 8, dtype=torch.float64, device=dev)
        bt_len = clip_length_table(ds).to(dev)
        bt_args = dict(distance=cfg.data.beat_distance, prominence_permille=beat_prominence_permille(cfg))
        file_ef = getattr(ds, "file_ef", None)
        if file_ef is not None:                                   # per cent per clip, NaN where a file has none
            file_ef = torch.tensor([float("nan") if (v := file_ef(k)) is None else float(v) for k in range(len(ds))], dtype=torch.float64).to(dev)
    bp_on = cfg.data.lv_biplane                                   # off: no new call below
    if bp_on:
        pair_tab = view_pair_table(ds)
        missing = [what for what, absent in (("data.lv_class >= 0", lv_cls < 0), ("a pixel spacing for every clip", not mm),
                                             ("a dataset that names every clip's patient and view", pair_tab is None)) if absent]
        if missing:
            raise SystemExit(f"eval.py: data.lv_biplane needs {' and '.join(missing)}")
        bp_pairs, bp_single = pair_tab                            # host int32 [P, 2] = (2CH clip, 4CH clip), patients with one view only
        # ops.lv_measure_mm's three records (stats, disks, geom) of EVERY clip of the split, of the post-processed prediction and of the
        # target: zeros until the clip's own batch writes its rows (a rank writes its shard's rows only, and a row of zeros is an empty frame)
        bp_rows = lambda: [torch.zeros(len(ds), cfg.data.frames, w, dtype=dt, device=dev)
                           for w, dt in ((12, torch.int64), (20, torch.int64), (6, torch.float64))]
        bp_pred, bp_tgt = bp_rows(), bp_rows()
    st_on = cfg.data.lv_strain                                    # off: no new call below (config: on needs lv_class >= 0)
    if st_on:
        st_args = dict(cls=lv_cls, wall=cfg.data.lv_wall_classes, base=cfg.data.lv_base_classes)
        # ops.ef_summary of the GLS [8], of the long-axis shortening [8], then the clips with a strain and without landmarks
        st_sums = torch.zeros(17, dtype=torch.float64, device=dev)
    nat_on = cfg.data.native_eval                                 # off: no new call below
    ns_cls = cfg.data.native_surface_class if nat_on else -1      # -1 = off: no new call below (config: >= 0 needs native_eval)
    if nat_on:
        nat_sizes = native_target_table(ds)                       # host int32 [clips, 2] = (h0, w0)
        if nat_sizes is None:
            raise SystemExit("eval.py: data.native_eval needs a dataset with a native target for every clip (camus_png written with "
                             "tools/convert_camus.py --native-masks, or npy_clips with a native_target array), each side in 1..2048")
        nat_post = bool(vote or keep or fillc)                    # a second set of sums for the post-processed mask
        nat_k = cfg.data.num_classes * 3 + 2                      # native counts [ncls, 3], then the pixels compared and the labelled frames
        nat_acc = torch.zeros((2 if nat_post else 1) * nat_k, dtype=torch.int64, device=dev)
        if ns_cls >= 0:
            # host int32 [clips, 2] micrometres per NATIVE pixel; without one for every clip the distances are in native pixels
            nat_sp = native_spacing_table(ds, cfg)
            ns_unit = "mm" if nat_sp is not None else "px"
            if nat_sp is None:
                nat_sp = torch.full((len(ds), 2), 1000, dtype=torch.int32)
            ns_sums = torch.zeros(5, dtype=torch.float64, device=dev)     # ops.surface_summary, accumulated on the device
    nlv_on = cfg.data.native_lv                                   # off: no new call below (config: on needs native_eval and lv_class >= 0)
    if nlv_on:
        # host int32 [clips, 2] micrometres per NATIVE pixel; without one for every clip the volumes are in native pixel^3
        nlv_sp = native_spacing_table(ds, cfg)
        nlv_unit = "mL" if nlv_sp is not None else "px3"
        if nlv_sp is None:
            nlv_sp = torch.full((len(ds), 2), 1000, dtype=torch.int32)
        # ops.ef_summary of the EF, the EDV and the ESV measured at native size [24], then the frames measured
        nlv_sums = torch.zeros(25, dtype=torch.float64, device=dev)
    vis_left = cfg.eval_stage.num_vis if rank == 0 else 0
    # this rank's shard through a prefetching loader (worker processes decode, pinned staging, host-to-device copies on a side stream) into
    # ONE captured forward per batch shape (SegmentRunner -> GraphedSegment: a hipGraph replay per batch; the short last batch runs eagerly)
    dl = torch.utils.data.DataLoader(torch.utils.data.Subset(ds, range(lo, hi)), batch_size=cfg.batch_size, shuffle=False, num_workers=2, pin_memory=True)
    fdt = torch.bfloat16 if cfg.precision == "bf16" else torch.float32
    runner = SegmentRunner(model, graph=os.environ.get("GDKVM_FWD_GRAPH", "1") != "0", in_flight=int(os.environ.get("GDKVM_FWD_IN_FLIGHT", "2")))
    i = lo

    def batches():
        """(mask, counts, target's LV measurement) per batch, one batch behind the submissions: the host queues batch i + 1 (copy, cast, replay)
        before it reads batch i's result, and two forwards are in flight (SegmentRunner(in_flight=2); GDKVM_FWD_IN_FLIGHT=1: one at a time).
        The TARGET is measured right behind the submission, on the stream where the prefetcher handed it out: its slot is recycled once the
        consumer asks for the next batch, so nothing may read it later -- the temporal vote of the prediction, its largest-component filter, its
        hole filling and its surface distances, one batch behind, want the target and get a copy made here.  The last element is the
        target's volumes in mL (with a spacing and lv_class >= 0): the loader is unshuffled, so the clips of a submission are the next rows
        of the spacing table; behind it, with data.lv_strain, the target's contour lengths."""
        pending = None
        sub = lo                                                  # the first clip of the batch being submitted
        for frames, target in DevicePrefetcher(dl, dev, slots=3, frames_dtype=fdt, target_dtype=torch.uint8):
            nxt = runner.submit(frames, target)
            t_copy = target.clone() if vote or keep or fillc or s_cls >= 0 else None
            if lv_cls >= 0:
                t_stats, _, t_geom = ops.lv_measure(target, cls=lv_cls)
                t_rec = ops.lv_measure_mm(target, spacing[sub:sub + target.shape[0], None], cls=lv_cls) if mm else None
                t_ml = t_rec[2][..., 1].contiguous() if mm else None
                if bp_on:                                         # the target's records at the clips' own rows
                    for tab, rec in zip(bp_tgt, t_rec):
                        tab[sub:sub + target.shape[0]] = rec
                t_len = None
                if st_on:                                         # the target's contour lengths [B, T, 3], mm with a spacing
                    t_sp = spacing[sub:sub + target.shape[0], None] if mm else None
                    t_len = ops.contour_lengths(ops.lv_contour(target, spacing_um=t_sp, **st_args), t_sp)
                nxt = (nxt, t_geom[..., 1].contiguous(), t_stats[..., 0].contiguous(), t_copy, t_ml, t_len)
            else:
                nxt = (nxt, None, None, t_copy, None, None)
            sub += target.shape[0]
            if pending is not None:
                yield pending[0].get() + pending[1:]
            pending = nxt
        if pending is not None:
            yield pending[0].get() + pending[1:]

    for mask, c, t_vol, t_npix, t_copy, t_ml, t_len in batches():
        sp = spacing[i:i + mask.shape[0], None] if mm else None   # [B, 1, 2]: results arrive one batch behind, in order, and i counts them
        # only frames that carry labels count (EchoNet-Dynamic: the two traced frames of a clip -- gdkvm_amd.data.IGNORE_LABEL everywhere
        # else, where a predicted pixel must not enter |A|): a labelled frame has a non-empty target in some class
        labelled = (c[..., 2].sum(-1, keepdim=True) > 0).unsqueeze(-1)
        measured, c_meas = mask, c                                # what is post-processed and measured, and its counts
        if vote:
            measured, tv, c_meas = ops.temporal_vote(mask, cfg.data.num_classes, vote, target=t_copy)
            tv_acc += ops.vote_summary(tv, c_meas, labelled[..., 0, 0])
        if keep:
            measured, lc = ops.largest_component(measured, cls=lv_cls, connectivity=keep, fill=0, target=t_copy)
            removed = (lc[..., 1] - lc[..., 2]).long()
            lc_acc += torch.cat([(ops.counts_after_largest(c_meas, lc, lv_cls, 0) * labelled).sum((0, 1)).long().reshape(-1),
                                 torch.stack([(removed > 0).sum(), removed.sum()])])
        if fillc:
            measured, fh = ops.fill_holes(measured, cls=lv_cls, connectivity=fillc, max_area=cfg.data.lv_fill_max_area, target=t_copy)
            fh_acc += torch.cat([(ops.class_counts_after_fill(fh) * labelled[..., 0]).sum((0, 1)),
                                 torch.stack([(fh[..., 3] > 0).sum(), fh[..., 0].clamp(min=0).sum(), fh[..., 3].sum()]).long()])
        if nat_on:
            # this batch's native targets, packed on the host (results arrive one batch behind, in order, and i counts them) and counted against
            # the raw mask -- and the post-processed one -- at every clip's own size; a frame counts when its native target has a class pixel
            nb = mask.shape[0]
            n_flat, n_sz = ops.pack_native([ds.native_target(k) for k in range(i, i + nb)])
            if n_sz != [tuple(r) for r in nat_sizes[i:i + nb].tolist()]:
                raise SystemExit(f"eval.py: the native targets of clips {i}..{i + nb - 1} do not have the sizes the dataset states")
            n_flat = n_flat.to(dev)
            n_px = torch.tensor([h0 * w0 for h0, w0 in n_sz], dtype=torch.int64, device=dev)
            for slot, pm in enumerate((mask, measured) if nat_post else (mask,)):
                lv_slot = nlv_on and slot == int(nat_post)        # the post-processed mask's slot (the raw one's without post-processing)
                n_out, n_c, _ = ops.mask_to_native(pm, n_sz, cfg.data.num_classes, target=n_flat,
                                                   want_out=(slot == 0 and ns_cls >= 0) or lv_slot)
                n_lab = n_c[..., 2].sum(-1) > 0                   # [B, T]
                if lv_slot:
                    # the volumes of that native mask and of the native target at every clip's own size; ED / ES are the target's frames,
                    # picked on the target's curve, and a clip counts when its target has two such frames and a volume, as for lv_mm
                    l_sp = nlv_sp[i:i + nb]
                    g_stats, _, g_geom = ops.lv_measure_native(n_flat, n_sz, mask.shape[1], l_sp, cls=lv_cls)
                    q_stats, _, q_geom = ops.lv_measure_native(n_out, n_sz, mask.shape[1], l_sp, cls=lv_cls)
                    g_vol, g_npix = g_geom[..., 1].contiguous(), g_stats[..., 0].contiguous()
                    g_idx, g_val = ops.lv_ef(g_vol, g_npix)
                    _, q_val = ops.lv_ef(q_geom[..., 1].contiguous(), q_stats[..., 0].contiguous(), pick_vol=g_vol, pick_npix=g_npix)
                    ok = (g_idx[:, 0] >= 0) & (g_val[:, 0] > 0)
                    nlv_sums += torch.cat([ops.ef_summary(q_val[:, k], g_val[:, k], ok) for k in (2, 0, 1)]
                                          + [torch.tensor([g_npix.numel()], dtype=torch.float64, device=dev)])
                if n_out is not None and slot == 0 and ns_cls >= 0:    # the raw mask's surface distances at native size, over the same frames
                    n_surf = ops.surface_distance_native(n_out, n_flat, n_sz, mask.shape[1], nat_sp[i:i + nb], cls=ns_cls)
                    ns_sums += ops.surface_summary(*ops.surface_metrics_mm(n_surf), n_surf, n_lab)
                nat_acc[slot * nat_k:(slot + 1) * nat_k] += torch.cat([(n_c * n_lab[..., None, None]).sum((0, 1)).long().reshape(-1),
                                                                       torch.stack([(n_lab.sum(1) * n_px).sum(), n_lab.sum()])])
        if lv_cls >= 0:
            # the prediction's volumes at the TARGET's end-diastolic / end-systolic frames (EchoNet-Dynamic: the two traced frames; unlabelled
            # frames hold no pixel of the class and are no candidates); a clip counts when its target has two such frames and a volume
            p_stats, _, p_geom = ops.lv_measure(measured, cls=lv_cls)
            r_idx, r_val = ops.lv_ef(t_vol, t_npix)
            _, p_val = ops.lv_ef(p_geom[..., 1], p_stats[..., 0], pick_vol=t_vol, pick_npix=t_npix)
            ef_sums[:8] += ops.ef_summary(p_val[:, 2], r_val[:, 2], (r_idx[:, 0] >= 0) & (r_val[:, 0] > 0))
            if mm:
                # the same post-processed mask and the same rule in mL: ED / ES are the target's frames, picked on the target's mL curve
                q_stats, q_disks, q_geom = ops.lv_measure_mm(measured, sp, cls=lv_cls)
                if bp_on:                                         # the prediction's records at the clips' own rows
                    for tab, rec in zip(bp_pred, (q_stats, q_disks, q_geom)):
                        tab[i:i + mask.shape[0]] = rec
                m_idx, m_val = ops.lv_ef(t_ml, t_npix)
                _, q_val = ops.lv_ef(q_geom[..., 1], q_stats[..., 0], pick_vol=t_ml, pick_npix=t_npix)
                ok = (m_idx[:, 0] >= 0) & (m_val[:, 0] > 0)
                ef_sums[8:] += torch.cat([ops.ef_summary(q_val[:, k], m_val[:, k], ok) for k in (2, 0, 1)])
            if st_on:
                # the contour of the same post-processed mask, read at the target's ED / ES frames as picked above (mm: on the mL curve);
                # a clip counts when the block above counts it and both sides have a contour at both frames
                s_rec = ops.lv_contour(measured, spacing_um=sp, **st_args)
                s_len = ops.contour_lengths(s_rec, sp)
                s_npix = s_rec[..., 0].contiguous()
                picks, use = (m_idx, ok) if mm else (r_idx, (r_idx[:, 0] >= 0) & (r_val[:, 0] > 0))
                parts = []
                for k in (0, 2):                                  # the endocardial contour, then the apex-to-annulus axis
                    _, g_ref, _, g_ok = ops.lv_strain(t_len[..., k].contiguous(), t_npix, picks)
                    _, g_pred, _, p_ok = ops.lv_strain(s_len[..., k].contiguous(), s_npix, picks)
                    parts.append(use & g_ok & p_ok & (parts[0] if parts else True))
                    st_sums[4 * k:4 * k + 8] += ops.ef_summary(g_pred[:, 0], g_ref[:, 0], parts[-1])
                st_sums[16] += (parts[0] & ~parts[1]).sum()
        if beats_on:
            # beat by beat, on the curves of the same post-processed mask: the prediction's, and the target's where it labels every valid frame
            ln = bt_len[i:i + mask.shape[0]]
            _, _, b_info, b_summ = ops.lv_beats(p_stats[..., 0], (q_geom if mm else p_geom)[..., 1], ln, **bt_args)
            _, _, r_info, r_summ = ops.lv_beats(t_npix, t_ml if mm else t_vol, ln, **bt_args)
            full = (labelled[..., 0, 0] | (torch.arange(mask.shape[1], device=dev) >= ln[:, None])).all(1)
            kept = b_info[:, 2] == 0
            cyc = kept & (b_info[:, 1] >= 2)
            bt_acc[:6] += torch.stack([torch.ones_like(kept).sum(), (~kept).sum(), kept.sum(), (b_info[:, 0] * kept).sum(), cyc.sum(),
                                       (b_summ[:, 3] * cyc).sum()]).to(torch.float64)
            bt_acc[6:17] += ops.beats_summary(b_summ, b_info, r_summ, r_info, ok=full)
            if file_ef is not None:
                fe = file_ef[i:i + mask.shape[0]]
                bt_acc[17:] += ops.ef_summary(b_summ[:, 0], torch.nan_to_num(fe) / 100.0, kept & (b_info[:, 0] >= 1) & ~torch.isnan(fe))
        if s_cls >= 0:
            surf = ops.surface_distance(mask, t_copy, cls=s_cls)
            sd_sums[:5] += ops.surface_summary(*ops.surface_metrics(surf), surf, labelled[..., 0, 0])
            if mm:
                surf = ops.surface_distance_mm(mask, t_copy, sp, cls=s_cls)
                sd_sums[5:] += ops.surface_summary(*ops.surface_metrics_mm(surf), surf, labelled[..., 0, 0])
        counts += (c * labelled).sum((0, 1)).long()
        if vis_left > 0:
            from PIL import Image
            os.makedirs(os.path.join(cfg.run_dir, "vis"), exist_ok=True)
            scale = 255 // max(cfg.data.num_classes - 1, 1)
            Image.fromarray((mask[0, 0].cpu().numpy() * scale).astype("uint8")).save(os.path.join(cfg.run_dir, "vis", f"mask_{i:05d}.png"))
            if cfg.eval_stage.vis_overlay:
                # clip i once more from the dataset (bytes: as_uint8; no prefetcher slot is held): plane 0 of its frames under the
                # post-processed mask, the target's contour as reference, every frame
                from gdkvm_amd.predict import overlay_clip
                v_frames, v_target = ds[i]
                pictures = overlay_clip(v_frames[:, 0].contiguous(), measured[0], cfg, reference=v_target).cpu().numpy()
                for t, pic in enumerate(pictures):
                    Image.fromarray(pic).save(os.path.join(cfg.run_dir, "vis", f"overlay_{i:05d}_{t:03d}.png"))
            vis_left -= 1
        i += mask.shape[0]
    if world > 1:
        torch.distributed.all_reduce(counts)                      # the only exchanges: 3 integers per class ...
        if lv_cls >= 0:
            torch.distributed.all_reduce(ef_sums)                 # ... and the eight EF sums
        if st_on:
            torch.distributed.all_reduce(st_sums)                 # ... and the strain sums
        if vote:
            torch.distributed.all_reduce(tv_acc)                  # ... and the voted mask's counts and change totals
        if keep:
            torch.distributed.all_reduce(lc_acc)                  # ... and the filtered mask's counts and removal totals
        if fillc:
            torch.distributed.all_reduce(fh_acc)                  # ... and the filled mask's counts and totals
        if s_cls >= 0:
            torch.distributed.all_reduce(sd_sums)                 # ... and the five surface-distance sums
        if beats_on:
            torch.distributed.all_reduce(bt_acc)                  # ... and the beat-by-beat sums
        if nat_on:
            torch.distributed.all_reduce(nat_acc)                 # ... and the native counts, pixels and frames
            if ns_cls >= 0:
                torch.distributed.all_reduce(ns_sums)             # ... and the five native surface-distance sums
            if nlv_on:
                torch.distributed.all_reduce(nlv_sums)            # ... and the native volume sums
        if bp_on:
            for tab in bp_pred + bp_tgt:                          # ... and the record tables: every row was written by one rank and is 0 on
                torch.distributed.all_reduce(tab)                 # the others, and integer and fp64 sums with zeros are exact
    if rank == 0:
        dice = ops.dice_from_counts(counts).tolist()
        iou = ops.iou_from_counts(counts).tolist()
        res = {"split": args.split, "clips": len(ds), "forward": {"graph_replays": runner.replays, "eager_calls": runner.eager_calls},
               "dice_per_class": [round(d, 5) for d in dice],
               "mean_foreground_dice": round(sum(dice[1:]) / max(len(dice) - 1, 1), 5),
               "iou_per_class": [round(d, 5) for d in iou],
               "mean_foreground_iou": round(sum(iou[1:]) / max(len(iou) - 1, 1), 5)}
        if lv_cls >= 0:
            res["lv"] = {k: (v if isinstance(v, int) else round(v, 5)) for k, v in ops.ef_stats(ef_sums[:8].cpu()).items()}
            if mm:
                acc = ef_sums.cpu()
                lv_mm = ops.ef_stats(acc[8:16])
                for name, sums in (("edv", acc[16:24]), ("esv", acc[24:32])):     # ef_summary's sums: count, sum e, sum |e|, ...
                    cnt = max(float(sums[0]), 1.0)
                    lv_mm[f"{name}_mae_ml"], lv_mm[f"{name}_bias_ml"] = float(sums[2]) / cnt, float(sums[1]) / cnt
                res["lv_mm"] = {k: (v if isinstance(v, int) else round(v, 5)) for k, v in lv_mm.items()}
            if st_on:
                acc = st_sums.cpu()
                names = {"clips_with_ef": "clips_with_strain", "ef_mae": "gls_mae", "ef_bias": "gls_bias", "ef_pearson_r": "gls_pearson_r",
                         "mean_ref_ef": "mean_ref_gls", "mean_pred_ef": "mean_pred_gls"}
                axis = {"clips_with_ef": "clips_with_landmarks", "ef_mae": "shortening_mae", "ef_bias": "shortening_bias",
                        "ef_pearson_r": "shortening_pearson_r", "mean_ref_ef": "mean_ref_shortening", "mean_pred_ef": "mean_pred_shortening"}
                rnd5 = lambda v: v if isinstance(v, int) else round(v, 5)
                blk = {"unit": "mm" if mm else "px", "wall_classes": list(cfg.data.lv_wall_classes), "base_classes": list(cfg.data.lv_base_classes),
                       **{names[k]: rnd5(v) for k, v in ops.ef_stats(acc[:8]).items()}}
                if cfg.data.lv_base_classes:
                    blk["long_axis"] = {**{axis[k]: rnd5(v) for k, v in ops.ef_stats(acc[8:16]).items()}, "clips_without_landmarks": int(acc[16])}
                else:
                    blk["long_axis"] = "none: data.lv_base_classes is empty, the strain is that of the whole outline and there are no landmarks"
                res["strain"] = blk
        if vote:
            acc = tv_acc.cpu()
            tv_dice = ops.dice_from_counts(acc[:-5].view(cfg.data.num_classes, 3)).tolist()
            nfr = max(int(acc[-1]), 1)
            res["temporal_vote"] = {"radius": vote, "frames_changed": int(acc[-4]), "pixels_changed": int(acc[-5]),
                                    "flips_per_frame_before": round(int(acc[-3]) / nfr, 5), "flips_per_frame_after": round(int(acc[-2]) / nfr, 5),
                                    "dice_per_class": [round(d, 5) for d in tv_dice],
                                    "mean_foreground_dice": round(sum(tv_dice[1:]) / max(len(tv_dice) - 1, 1), 5)}
        if keep:
            acc = lc_acc.cpu()
            lc_counts = acc[:-2].view(cfg.data.num_classes, 3)
            res["largest_component"] = {"connectivity": keep, "frames_changed": int(acc[-2]), "pixels_removed": int(acc[-1]),
                                        "dice_lv": round(float(ops.dice_from_counts(lc_counts)[lv_cls]), 5),
                                        "iou_lv": round(float(ops.iou_from_counts(lc_counts)[lv_cls]), 5)}
        if fillc:
            acc = fh_acc.cpu()
            res["fill_holes"] = {"connectivity": fillc, "max_area": cfg.data.lv_fill_max_area, "frames_changed": int(acc[3]), "holes": int(acc[4]),
                                 "pixels_filled": int(acc[5]), "dice_lv": round(float(ops.dice_from_counts(acc[:3])), 5),
                                 "iou_lv": round(float(ops.iou_from_counts(acc[:3])), 5)}
        if s_cls >= 0:
            res["surface"] = {"class": s_cls, **{k: (v if isinstance(v, int) else round(v, 5)) for k, v in ops.surface_stats(sd_sums[:5].cpu()).items()}}
            if mm:
                st = ops.surface_stats(sd_sums[5:].cpu())
                res["surface_mm"] = {"frames": st["frames"], "frames_one_empty": st["frames_one_empty"],
                                     **{k + "_mm": round(st[k], 5) for k in ("hd_mean", "hd95_mean", "assd_mean")}}
        if beats_on:
            acc = bt_acc.cpu()
            r5 = lambda v: round(float(v), 5)
            vs_t = ops.beats_stats(acc[6:17])
            res["beats"] = {"clips": int(acc[0]), "beats_per_clip": r5(acc[3] / max(float(acc[2]), 1.0)),
                            "mean_cycle_frames": r5(acc[5] / max(float(acc[4]), 1.0)), "clips_dropped_below_min": int(acc[1]),
                            "clips_with_target": vs_t["clips"], "ef_mae": r5(vs_t["ef_mae"]), "ef_bias": r5(vs_t["ef_bias"]),
                            "ef_pearson_r": r5(vs_t["ef_pearson_r"]), "systole_count_agreement": r5(vs_t["systole_count_agreement"])}
            if file_ef is not None:
                vs_f = ops.ef_stats(acc[17:])
                res["beats"]["vs_file_ef"] = {k: (v if isinstance(v, int) else r5(v)) for k, v in vs_f.items()
                                              if k in ("clips_with_ef", "ef_mae", "ef_bias", "ef_pearson_r")}
        if bp_on:
            # one launch per side over the whole split's tables; ED / ES are the target's frames, picked on its bi-plane curve
            rnd = lambda v: v if isinstance(v, int) else round(float(v), 5)
            g_out, g_npix = ops.lv_biplane(*bp_tgt, spacing[:, None], bp_pairs)
            p_out, p_npix = ops.lv_biplane(*bp_pred, spacing[:, None], bp_pairs)
            g_vol = g_out[..., 0].contiguous()
            g_idx, g_val = ops.lv_ef(g_vol, g_npix)
            _, p_val = ops.lv_ef(p_out[..., 0].contiguous(), p_npix, pick_vol=g_vol, pick_npix=g_npix)
            ok = (g_idx[:, 0] >= 0) & (g_val[:, 0] > 0)           # the pairs with a target: two valid frames and an EDV
            # sums of (predicted - reference) and of its magnitude over the pairs where `use`, as MAE and bias
            def mae_bias(p, g, use):
                s = ops.ef_summary(p, g, use).cpu()
                cnt = max(float(s[0]), 1.0)
                return float(s[2]) / cnt, float(s[1]) / cnt
            blk = {"pairs": int(bp_pairs.shape[0]), "patients_single_view": int(bp_single), "pairs_with_target": int(ok.sum()),
                   **ops.ef_stats(ops.ef_summary(p_val[:, 2], g_val[:, 2], ok).cpu())}
            for name, k in (("edv", 0), ("esv", 1)):
                blk[f"{name}_mae_ml"], blk[f"{name}_bias_ml"] = mae_bias(p_val[:, k], g_val[:, k], ok)
            # the two long axes of the PREDICTION at end-diastole: the guidelines want them within 10 % of each other
            mism = p_out[..., 2].gather(1, g_idx[:, :1].clamp(min=0).long())[:, 0] * ok
            blk["length_mismatch_mean"] = float(mism.sum()) / max(int(ok.sum()), 1)
            blk["pairs_length_mismatch_over_10pct"] = int((mism > 0.1).sum())
            info = getattr(ds, "info", None)
            if info is not None:
                # what the files state per patient (CAMUS: bi-plane Simpson values), from the 2CH view's info, else the 4CH view's
                def stated(key, scale):
                    vals = []
                    for a, b in bp_pairs.tolist():
                        got = [v for v in ((info(c) or {}).get(key) for c in (a, b))
                               if isinstance(v, (int, float)) and not isinstance(v, bool) and v == v and abs(v) != float("inf")]
                        if len(got) == 2 and got[0] != got[1]:
                            print(f"eval.py: biplane: {key} of clips {a} (2CH) and {b} (4CH) differ: {got[0]} and {got[1]}; the 2CH value is used",
                                  file=sys.stderr, flush=True)
                        vals.append(float(got[0]) * scale if got else float("nan"))
                    return torch.tensor(vals, dtype=torch.float64).reshape(len(vals)).to(dev)
                f_ef = stated("ef_percent", 0.01)
                have = ok & ~torch.isnan(f_ef)
                f_ef = torch.nan_to_num(f_ef)
                vs = {"pairs_with_ef": int(have.sum()),
                      **{k: v for k, v in ops.ef_stats(ops.ef_summary(p_val[:, 2], f_ef, have).cpu()).items() if k in ("ef_mae", "ef_bias", "ef_pearson_r")},
                      "target_ef_mae": mae_bias(g_val[:, 2], f_ef, have)[0]}
                for name, k in (("edv", 0), ("esv", 1)):
                    f_v = stated(f"{name}_ml", 1.0)
                    have = ok & ~torch.isnan(f_v)
                    f_v = torch.nan_to_num(f_v)
                    vs[f"pairs_with_{name}"] = int(have.sum())
                    vs[f"{name}_mae_ml"], vs[f"{name}_bias_ml"] = mae_bias(p_val[:, k], f_v, have)
                    vs[f"target_{name}_mae_ml"] = mae_bias(g_val[:, k], f_v, have)[0]
                blk["vs_file"] = {k: rnd(v) for k, v in vs.items()}
            res["biplane"] = {k: (v if isinstance(v, dict) else rnd(v)) for k, v in blk.items()}
        if nat_on:
            def nat_block(acc):
                n_counts = acc[:-2].view(cfg.data.num_classes, 3)
                n_dice, n_iou = ops.dice_from_counts(n_counts).tolist(), ops.iou_from_counts(n_counts).tolist()
                return {"dice_per_class": [round(d, 5) for d in n_dice],
                        "mean_foreground_dice": round(sum(n_dice[1:]) / max(len(n_dice) - 1, 1), 5),
                        "iou_per_class": [round(d, 5) for d in n_iou],
                        "mean_foreground_iou": round(sum(n_iou[1:]) / max(len(n_iou) - 1, 1), 5),
                        "pixels": int(acc[-2]), "frames": int(acc[-1])}
            acc = nat_acc.cpu()
            res["native"] = nat_block(acc[:nat_k])
            if nat_post:
                res["native"]["post"] = nat_block(acc[nat_k:])
            if ns_cls >= 0:
                st = ops.surface_stats(ns_sums.cpu())
                res["native"]["surface"] = {"class": ns_cls, "unit": ns_unit, "frames": st["frames"], "frames_one_empty": st["frames_one_empty"],
                                            **{k: round(st[k], 5) for k in ("hd_mean", "hd95_mean", "assd_mean")}}
            if nlv_on:
                acc = nlv_sums.cpu()
                blk = ops.ef_stats(acc[:8])
                if nlv_unit == "mL":                              # (in pixel^3 the EF, a ratio, is all there is to report)
                    for name, sums in (("edv", acc[8:16]), ("esv", acc[16:24])):
                        cnt = max(float(sums[0]), 1.0)
                        blk[f"{name}_mae_ml"], blk[f"{name}_bias_ml"] = float(sums[2]) / cnt, float(sums[1]) / cnt
                res["native"]["lv"] = {**{k: (v if isinstance(v, int) else round(v, 5)) for k, v in blk.items()}, "unit": nlv_unit,
                                       "frames": int(acc[24])}
        print(json.dumps(res), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
