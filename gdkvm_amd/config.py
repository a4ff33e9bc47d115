"""Run configuration: a small typed mirror of the reference harness's YAML (hydra / omegaconf are not available here).

Key names are the ones the reference's reproduction guide shows (``data_path, batch_size, learning_rate, num_iterations,
eval_stage.num_vis, eval_stage.wandb_mode`` -- /root/reference/website/src/pages/[lang]/reprod/index.astro:246-252); the
launcher environment variables are torchrun's (``MASTER_PORT`` etc., index.astro:238-239)."""
from __future__ import annotations

import math
from dataclasses import asdict, dataclass, field, fields, is_dataclass
from typing import Any, Dict, List, Optional

import yaml


@dataclass
class EvalStage:
    num_vis: int = 0
    wandb_mode: str = "offline"
    vis_overlay: bool = False        # eval.py: beside every vis/mask_XXXXX.png, vis/overlay_XXXXX_TTT.png of every frame of that clip: the
                                     # post-processed mask over the frame, the target's contour as reference (predict.overlay_clip)


@dataclass
class DataCfg:
    kind: str = "synthetic"          # synthetic | npy_clips | echonet_npz | camus_png
    frames: int = 10
    size: int = 256
    num_classes: int = 4
    lv_class: int = 1                # eval.py: the class whose volumes and ejection fraction are measured (ops.lv_measure / lv_ef); -1 = off
    lv_keep_largest: int = 0         # eval.py: keep the largest connected component of lv_class in the PREDICTED mask before it is measured
                                     # (ops.largest_component, fill = 0); 0 = off, 4 or 8 = the connectivity
    lv_fill_holes: int = 0           # eval.py: fill the holes of lv_class in the PREDICTED mask (after lv_keep_largest) before it is measured
                                     # (ops.fill_holes); 0 = off, 4 or 8 = the connectivity of the class's COMPLEMENT
    lv_fill_max_area: int = 0        # ... only the holes of at most this many pixels; 0 = holes of any size
    temporal_vote: int = 0           # eval.py: smooth the PREDICTED masks of a clip over time before anything above (ops.temporal_vote: per-pixel
                                     # majority over the frames t - r .. t + r); 0 = off, 1..7 = the radius r
    surface_class: int = -1          # eval.py: the class whose HD, HD95 and ASSD against the target are measured (ops.surface_distance, pixels of
                                     # the input grid); -1 = off
    spacing_um: Any = None           # eval.py: [row_um, col_um], the micrometres per pixel of the network grid (integers in 1..4095) for datasets
                                     # that carry no spacing of their own (data.clip_spacing_table); with a spacing eval.py adds the mL / mm blocks
    lv_beats: bool = False           # eval.py: beat-by-beat EF of lv_class from the whole clip's area curve (ops.lv_beats): a `beats` block
    beat_distance: int = 20          # ... the fewest frames between two end-systoles, 1..4096 (find_peaks' distance=; EchoNet-Dynamic: 20 at 50 fps)
    beat_prominence: float = 0.5     # ... the prominence an end-systole needs, as a fraction 0..1 of the curve's range (handed on in per mille)
    lv_biplane: bool = False         # eval.py: bi-plane Simpson volumes and EF per patient from its 2CH and 4CH clips (ops.lv_biplane): a `biplane`
                                     # block; needs lv_class >= 0, a spacing for every clip and a dataset with patient / view (camus_png)
    native_eval: bool = False        # eval.py: Dice / IoU at every clip's NATIVE frame size against the tracing as stored (ops.mask_to_native): a
                                     # `native` block; needs a dataset with a native target for every clip (data.native_target_table)
    native_surface_class: int = -1   # eval.py: the class whose HD, HD95 and ASSD are also measured at every clip's NATIVE frame size
                                     # (ops.surface_distance_native): a `surface` block inside `native`; -1 = off, >= 0 needs native_eval
    native_lv: bool = False          # eval.py, predict.py: EDV, ESV and EF of lv_class measured at every clip's NATIVE frame size
                                     # (ops.lv_measure_native): an `lv` block inside `native` / an `lv_native` entry per clip; needs native_eval
                                     # (eval.py) and lv_class >= 0
    native_spacing_um: Any = None    # eval.py: [row_um, col_um], the micrometres per NATIVE pixel (integers in 1..4095) for datasets that carry
                                     # none of their own (data.native_spacing_table); without a spacing for every clip the block is in pixels
    lv_strain: bool = False          # eval.py: global longitudinal strain of lv_class from its contour's length at ED and ES (ops.lv_contour /
                                     # contour_lengths / lv_strain): a `strain` block; needs lv_class >= 0
    lv_wall_classes: Any = field(default_factory=lambda: [2])    # ... the classes whose border with lv_class is the endocardium (non-empty)
    lv_base_classes: Any = field(default_factory=lambda: [3])    # ... the classes whose border with lv_class is the mitral plane: apex, long
                                     # axis and its shortening come from it.  A binary dataset sets [0] / []: the whole outline's strain, no landmarks
    synthetic_beats: float = 1.0     # the synthetic clips' heart beats per clip (> 0; 1.0: the clips of before, bit for bit)
    whole_video: bool = False        # echonet_npz only: a clip is the video's first `frames` frames (several beats), not the window around ED / ES


@dataclass
class ModelCfg:
    heads: int = 1
    key_dim: int = 64                # Dk per head: 64 runs the measured kernels; 72 .. 256 (multiples of 8) the wide-key coverage path
    value_dim: int = 256
    rule: str = "delta_sequential"
    scan_segments: int = 1           # evaluation of long clips: GDKVMConfig.scan_segments (1 = serial scan, bit-identical under chunking)
    mask_feedback: bool = False      # GDKVMConfig.mask_feedback: train and evaluate in the per-frame step mode (predicted masks fed back)


@dataclass
class AugmentCfg:
    """Training-clip augmentation on the GPU (data.ClipAugment -> gdkvm_augment_clips inside the prefetcher's cast pass).  Off by default;
    every range defaults to a no-op.  eval.py never augments."""
    enabled: bool = False
    rotate_deg: float = 0.0                                        # rotation in +-degrees about the frame centre
    scale: List[float] = field(default_factory=lambda: [1.0, 1.0])  # (lo, hi) zoom
    translate: float = 0.0                                         # shift as a +-fraction of the frame size
    hflip: float = 0.0                                             # probability of a left-right mirror
    gain: List[float] = field(default_factory=lambda: [1.0, 1.0])  # (lo, hi) intensity gain
    bias: float = 0.0                                              # +-intensity offset
    gamma: List[float] = field(default_factory=lambda: [1.0, 1.0])  # (lo, hi), log-uniform


@dataclass
class LossCfg:
    """The training objective beyond cross-entropy + soft Dice.  boundary_weight > 0 adds that many times the boundary loss of Kervadec et al.
    (train.segmentation_loss; on the GPU ops.seg_loss_boundary over ops.signed_distance).  The weight is a constant of the run."""
    boundary_weight: float = 0.0
    boundary_classes: Optional[List[int]] = None                   # null: every class but 0 (the term is not divided by their number)


@dataclass
class OptimCfg:
    """The optimiser.  kind: torch = torch.optim.AdamW (fused and capturable in the captured step), the run of before; native = optim.NativeAdamW
    (csrc/adamw.hip), which alone knows the keys from decay_1d on: under kind: torch they must keep their defaults, nothing is silently ignored.
    The schedule's total_steps is num_iterations."""
    kind: str = "torch"
    weight_decay: float = 0.01                                     # torch.optim.AdamW's own default
    betas: List[float] = field(default_factory=lambda: [0.9, 0.999])
    eps: float = 1e-8
    decay_1d: bool = True                                          # false: parameters with dim <= 1 (BatchNorm scales, every bias) get decay 0
    clip_norm: float = 0.0                                         # global gradient-norm clipping; 0 = off
    schedule: str = "constant"                                     # constant | cosine | poly, after warmup_steps of linear warm-up
    warmup_steps: int = 0
    min_lr_ratio: float = 0.0                                      # the schedule ends at learning_rate * min_lr_ratio
    poly_power: float = 0.9
    ema_decay: float = 0.0                                         # > 0: an EMA of the weights, saved as the checkpoint's "ema" (eval.py --ema)


@dataclass
class OverlayCfg:
    """How ops.overlay_native draws a mask over its frame (predict.py --overlay, eval_stage.vis_overlay)."""
    alpha: int = 96                                                # the class tint's weight out of 256: 0 = contours only, 256 = solid
    width: int = 2                                                 # the contour's width in pixels, 1..3
    palette: Optional[List[List[int]]] = None                      # null (ops.OVERLAY_PALETTE) or data.num_classes entries [r, g, b] in 0..255
    reference_palette: Optional[List[List[int]]] = None            # the same for a reference mask's contour (ops.OVERLAY_REFERENCE_PALETTE)


OPTIM_NATIVE_ONLY = ("decay_1d", "clip_norm", "schedule", "warmup_steps", "min_lr_ratio", "poly_power", "ema_decay")


@dataclass
class RunConfig:
    data_path: str = ""
    batch_size: int = 8
    learning_rate: float = 1.0e-4
    num_iterations: int = 3000
    eval_stage: EvalStage = field(default_factory=EvalStage)
    data: DataCfg = field(default_factory=DataCfg)
    model: ModelCfg = field(default_factory=ModelCfg)
    augment: AugmentCfg = field(default_factory=AugmentCfg)
    loss: LossCfg = field(default_factory=LossCfg)
    optim: OptimCfg = field(default_factory=OptimCfg)
    overlay: OverlayCfg = field(default_factory=OverlayCfg)
    run_dir: str = "outputs"
    save_every: int = 1000
    log_every: int = 20
    seed: int = 0
    precision: str = "bf16"

    def to_dict(self) -> Dict[str, Any]:
        return asdict(self)


def _build(cls, raw: Dict[str, Any]):
    known = {f.name: f for f in fields(cls)}
    unknown = set(raw) - set(known)
    if unknown:
        raise KeyError(f"unknown configuration key(s) for {cls.__name__}: {sorted(unknown)}")
    kw = {}
    for name, val in raw.items():
        ft = known[name].default_factory() if callable(getattr(known[name], "default_factory", None)) and \
            known[name].default_factory is not None and is_dataclass(known[name].default_factory()) else None
        kw[name] = _build(type(ft), val or {}) if ft is not None else val
    return cls(**kw)


def load_config(path: str | None = None, overrides: list[str] | None = None) -> RunConfig:
    """YAML file + ``key=value`` / ``a.b=value`` overrides (the hydra command-line style the reference uses)."""
    raw: Dict[str, Any] = {}
    if path:
        with open(path) as f:
            raw = yaml.safe_load(f) or {}
    for ov in overrides or []:
        key, _, val = ov.partition("=")
        if not _:
            raise ValueError(f"override {ov!r} is not key=value")
        node = raw
        parts = key.split(".")
        for p in parts[:-1]:
            node = node.setdefault(p, {})
        node[parts[-1]] = yaml.safe_load(val)
    cfg = _build(RunConfig, raw)
    cfg.learning_rate = float(cfg.learning_rate)
    if isinstance(cfg.data.lv_keep_largest, bool) or cfg.data.lv_keep_largest not in (0, 4, 8):
        raise ValueError(f"data.lv_keep_largest = {cfg.data.lv_keep_largest!r}: 0 (off), 4 or 8 (the connectivity)")
    if isinstance(cfg.data.lv_fill_holes, bool) or cfg.data.lv_fill_holes not in (0, 4, 8):
        raise ValueError(f"data.lv_fill_holes = {cfg.data.lv_fill_holes!r}: 0 (off), 4 or 8 (the connectivity of the class's complement)")
    fa = cfg.data.lv_fill_max_area
    if isinstance(fa, bool) or not isinstance(fa, int) or not 0 <= fa < 2 ** 31:
        raise ValueError(f"data.lv_fill_max_area = {fa!r}: an integer >= 0 (0 = holes of any size)")
    tv = cfg.data.temporal_vote
    if isinstance(tv, bool) or not isinstance(tv, int) or not 0 <= tv <= 7:
        raise ValueError(f"data.temporal_vote = {tv!r}: 0 (off) or the radius 1..7 of the vote's window")
    if tv and not 2 <= cfg.data.num_classes <= 8:
        raise ValueError(f"data.temporal_vote = {tv}: ops.temporal_vote votes over 2..8 classes, data.num_classes = {cfg.data.num_classes}")
    sc = cfg.data.surface_class
    if isinstance(sc, bool) or not isinstance(sc, int) or not -1 <= sc < cfg.data.num_classes:
        raise ValueError(f"data.surface_class = {sc!r}: -1 (off) or a class in 0..{cfg.data.num_classes - 1}")
    sp = cfg.data.spacing_um
    if sp is not None and (not isinstance(sp, list) or len(sp) != 2
                           or any(isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= 4095 for v in sp)):
        raise ValueError(f"data.spacing_um = {sp!r}: null or [row_um, col_um], two integers in 1..4095 (micrometres per pixel)")
    d = cfg.data
    if not isinstance(d.lv_beats, bool) or not isinstance(d.whole_video, bool):
        raise ValueError(f"data.lv_beats = {d.lv_beats!r}, data.whole_video = {d.whole_video!r}: true or false")
    if not isinstance(d.lv_biplane, bool):
        raise ValueError(f"data.lv_biplane = {d.lv_biplane!r}: true or false")
    if not isinstance(d.native_eval, bool):
        raise ValueError(f"data.native_eval = {d.native_eval!r}: true or false")
    if d.native_eval and not 2 <= d.num_classes <= 8:
        raise ValueError(f"data.native_eval: ops.mask_to_native votes over 2..8 classes, data.num_classes = {d.num_classes}")
    nsc = d.native_surface_class
    if isinstance(nsc, bool) or not isinstance(nsc, int) or not -1 <= nsc < d.num_classes:
        raise ValueError(f"data.native_surface_class = {nsc!r}: -1 (off) or a class in 0..{d.num_classes - 1}")
    if nsc >= 0 and not d.native_eval:
        raise ValueError(f"data.native_surface_class = {nsc} needs data.native_eval: true (the surface distances at native size are part of "
                         "the `native` block)")
    if not isinstance(d.native_lv, bool):
        raise ValueError(f"data.native_lv = {d.native_lv!r}: true or false")
    if d.native_lv and not (d.native_eval and d.lv_class >= 0):
        raise ValueError(f"data.native_lv needs data.native_eval: true and data.lv_class >= 0 (the volumes at native size are part of the "
                         f"`native` block and are those of lv_class), got native_eval = {d.native_eval}, lv_class = {d.lv_class}")
    nsp = d.native_spacing_um
    if nsp is not None and (not isinstance(nsp, list) or len(nsp) != 2
                            or any(isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= 4095 for v in nsp)):
        raise ValueError(f"data.native_spacing_um = {nsp!r}: null or [row_um, col_um], two integers in 1..4095 (micrometres per native pixel)")
    if not isinstance(d.lv_strain, bool):
        raise ValueError(f"data.lv_strain = {d.lv_strain!r}: true or false")
    for key in ("lv_wall_classes", "lv_base_classes"):
        cl = getattr(d, key)
        if not isinstance(cl, list) or any(isinstance(c, bool) or not isinstance(c, int) for c in cl) or len(set(cl)) != len(cl):
            raise ValueError(f"data.{key} = {cl!r}: a list of distinct class numbers")
    if d.lv_strain:                  # (the class lists are only read with the switch on: a binary dataset keeps the defaults while it is off)
        if d.lv_class < 0:
            raise ValueError("data.lv_strain needs data.lv_class >= 0 (the class whose contour is measured)")
        top = min(d.num_classes, 32) - 1
        for key in ("lv_wall_classes", "lv_base_classes"):
            cl = getattr(d, key)
            if any(not 0 <= c <= top for c in cl) or d.lv_class in cl:
                raise ValueError(f"data.{key} = {cl!r}: classes in 0..{top} other than data.lv_class = {d.lv_class}")
        if d.lv_class > top:
            raise ValueError(f"data.lv_strain: data.lv_class = {d.lv_class} outside 0..{top}")
        if not d.lv_wall_classes:
            raise ValueError("data.lv_wall_classes is empty: the contour needs at least one class on the other side "
                             "(a binary dataset: lv_wall_classes: [0], lv_base_classes: [])")
        if set(d.lv_wall_classes) & set(d.lv_base_classes):
            raise ValueError(f"data.lv_wall_classes = {d.lv_wall_classes!r} and data.lv_base_classes = {d.lv_base_classes!r} overlap")
    if d.whole_video and d.kind != "echonet_npz":
        raise ValueError(f"data.whole_video is for data.kind = echonet_npz, not {d.kind!r}")
    if isinstance(d.beat_distance, bool) or not isinstance(d.beat_distance, int) or not 1 <= d.beat_distance <= 4096:
        raise ValueError(f"data.beat_distance = {d.beat_distance!r}: an integer in 1..4096 (frames between two end-systoles)")
    bp = d.beat_prominence
    if isinstance(bp, bool) or not isinstance(bp, (int, float)) or not 0 <= bp <= 1:
        raise ValueError(f"data.beat_prominence = {bp!r}: a number in 0..1 (a fraction of the area curve's range)")
    d.beat_prominence = float(bp)
    sb = d.synthetic_beats
    if isinstance(sb, bool) or not isinstance(sb, (int, float)) or not math.isfinite(sb) or not sb > 0:
        raise ValueError(f"data.synthetic_beats = {sb!r}: a finite number > 0 (heart beats per synthetic clip)")
    d.synthetic_beats = float(sb)
    bw = cfg.loss.boundary_weight
    if isinstance(bw, bool) or not isinstance(bw, (int, float)) or not math.isfinite(bw) or bw < 0:
        raise ValueError(f"loss.boundary_weight = {bw!r}: a finite number >= 0 (0 = off)")
    cfg.loss.boundary_weight = float(bw)
    bc = cfg.loss.boundary_classes
    if bc is not None:
        if not isinstance(bc, list) or any(isinstance(c, bool) or not isinstance(c, int) or not 0 <= c < cfg.data.num_classes for c in bc) \
                or len(set(bc)) != len(bc):
            raise ValueError(f"loss.boundary_classes = {bc!r}: null (every class but 0) or distinct integers in 0..{cfg.data.num_classes - 1}")
    _check_optim(cfg.optim)
    if not isinstance(cfg.eval_stage.vis_overlay, bool):
        raise ValueError(f"eval_stage.vis_overlay = {cfg.eval_stage.vis_overlay!r}: true or false")
    if cfg.eval_stage.vis_overlay and not 2 <= d.num_classes <= 8:
        raise ValueError(f"eval_stage.vis_overlay: ops.overlay_native draws 2..8 classes, data.num_classes = {d.num_classes}")
    _check_overlay(cfg.overlay, d.num_classes)
    return cfg


def _check_overlay(o: OverlayCfg, num_classes: int) -> None:
    if isinstance(o.alpha, bool) or not isinstance(o.alpha, int) or not 0 <= o.alpha <= 256:
        raise ValueError(f"overlay.alpha = {o.alpha!r}: an integer in 0..256 (the tint's weight out of 256)")
    if isinstance(o.width, bool) or not isinstance(o.width, int) or not 1 <= o.width <= 3:
        raise ValueError(f"overlay.width = {o.width!r}: an integer in 1..3 (the contour's width in pixels)")
    for key in ("palette", "reference_palette"):
        pal = getattr(o, key)
        if pal is None:
            continue
        if not isinstance(pal, list) or any(not isinstance(c, list) or len(c) != 3 or any(isinstance(v, bool) or not isinstance(v, int)
                                                                                           or not 0 <= v <= 255 for v in c) for c in pal):
            raise ValueError(f"overlay.{key} = {pal!r}: null or a list of [r, g, b], integers in 0..255")
        if len(pal) != num_classes:
            raise ValueError(f"overlay.{key} has {len(pal)} colours, data.num_classes = {num_classes}: one [r, g, b] per class")


def beat_prominence_permille(cfg: RunConfig) -> int:
    """data.beat_prominence as the per-mille integer ops.lv_beats takes."""
    return int(round(cfg.data.beat_prominence * 1000))


def _check_optim(o: OptimCfg) -> None:
    num = lambda x: not isinstance(x, bool) and isinstance(x, (int, float)) and math.isfinite(x)
    if o.kind not in ("torch", "native"):
        raise ValueError(f"optim.kind = {o.kind!r}: torch or native")
    for key in ("weight_decay", "eps", "clip_norm", "poly_power", "min_lr_ratio", "ema_decay"):      # (YAML 1.1 reads 1e-8, without a dot, as a string)
        if isinstance(getattr(o, key), str):
            try:
                setattr(o, key, float(getattr(o, key)))
            except ValueError:
                pass
    for key in ("weight_decay", "eps", "clip_norm", "poly_power"):
        if not num(getattr(o, key)) or getattr(o, key) < 0:
            raise ValueError(f"optim.{key} = {getattr(o, key)!r}: a finite number >= 0")
        setattr(o, key, float(getattr(o, key)))
    if not isinstance(o.betas, list) or len(o.betas) != 2 or not all(num(b) and 0 <= b < 1 for b in o.betas):
        raise ValueError(f"optim.betas = {o.betas!r}: two numbers in [0, 1)")
    o.betas = [float(b) for b in o.betas]
    if not isinstance(o.decay_1d, bool):
        raise ValueError(f"optim.decay_1d = {o.decay_1d!r}: true or false")
    if o.schedule not in ("constant", "cosine", "poly"):
        raise ValueError(f"optim.schedule = {o.schedule!r}: constant, cosine or poly")
    if isinstance(o.warmup_steps, bool) or not isinstance(o.warmup_steps, int) or o.warmup_steps < 0:
        raise ValueError(f"optim.warmup_steps = {o.warmup_steps!r}: an integer >= 0")
    if not num(o.min_lr_ratio) or not 0 <= o.min_lr_ratio <= 1:
        raise ValueError(f"optim.min_lr_ratio = {o.min_lr_ratio!r}: a number in [0, 1]")
    o.min_lr_ratio = float(o.min_lr_ratio)
    if not num(o.ema_decay) or not 0 <= o.ema_decay < 1:
        raise ValueError(f"optim.ema_decay = {o.ema_decay!r}: a number in [0, 1) (0 = off)")
    o.ema_decay = float(o.ema_decay)
    if o.kind == "torch":
        default = OptimCfg()
        set_ = [k for k in OPTIM_NATIVE_ONLY if getattr(o, k) != getattr(default, k)]
        if set_:
            raise ValueError(f"optim.{set_[0]} = {getattr(o, set_[0])!r} needs optim.kind = native: torch.optim.AdamW has no such option "
                             f"(native-only keys: {', '.join(OPTIM_NATIVE_ONLY)})")
