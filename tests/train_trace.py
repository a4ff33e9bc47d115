"""One real bf16 training step, call by call: a tracer over the ``gdkvm_amd.ops`` entry points the training forward calls, the wiring of
those calls written down from the architecture (oracle/model_plain.py's _block_train / _up_train / plain_loss_and_grads), and a float64
reference of every entry point with its vector-Jacobian product.  Test infrastructure (tests/test_train_trace_*.py); not a conftest.

The point: bf16 module gradients compared end to end with a float64 restatement differ by 10-30 % per tensor (bf16 rounding flips,
amplified through BatchNorm backward), a bound that hides a wrong tap, a lost skip gradient or a stale weight pack.  Compared PER CALL,
on the very tensors the step produced (teacher-forced), every kernel is held to its own rounding bound.

    trace = StepTrace(model); with trace.installed(): train_step(...)   -> trace.calls: one Call per entry-point call
    wiring(cfg, B, T, H, W)                                             -> the graph: which recorded output feeds which input
    reference(entry, args, bf16, relu_mask)                             -> float64 outputs of one call (differentiable)
"""
from __future__ import annotations

import contextlib
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

# Every gdkvm_amd.ops function the training forward (GDKVM.forward under bf16 autocast, train mode, _lowres=True) and the fused
# objective (train.segmentation_loss_lowres) call at the default widths.  Positional layouts, as model.py / train.py call them:
ENTRY_POINTS = {
    "stem_conv": "x, weight",
    "bn_relu_pool": "x, weight, bias, running_mean, running_var, momentum, eps",
    "conv3x3_fork": "x, weight",
    "conv3x3": "x, weight",
    "conv_s2_block": "x, weight, down_weight",
    "bn_act": "x, weight, bias, running_mean, running_var, residual, momentum, eps, relu",
    "upsample_cat": "lo, skip",
    "token_projections": "x2d, w0, b0, w1, b1, ...  (the layers' weights and biases, expanded)",
    "scan": "q, k, v, alpha, beta, state, rule, flags",
    "kpff": "local, glob, pixel, wa, ba, wl, wg, h, w",
    "head": "x, weight, bias",
    "seg_loss": "z, target, dice_weight, eps",
}


# Calls per entry point in one training step of the default architecture (widths 64 / 128 / 256):
CENSUS = {
    "stem_conv": 1,           # the 7x7 / stride-2 stem convolution
    "bn_relu_pool": 1,        # the stem's BatchNorm + ReLU + max-pool
    "conv3x3_fork": 4,        # conv1 of the four identity blocks (layer1.0, layer1.1, layer2.1, layer3.1): input = convolution + skip
    "conv_s2_block": 2,       # conv1 + 1x1 downsample of the two strided blocks (layer2.0, layer3.0)
    "conv3x3": 10,            # conv2 of all six blocks, two convolutions in each of the two decoder stages
    "bn_act": 18,             # bn1 + bn2 of six blocks, down.1 of two, two per decoder stage (the 19th BatchNorm is the stem's)
    "upsample_cat": 2,        # decoder.up8 and decoder.up4
    "token_projections": 1,   # key / query / value / write gate / decay of the stride-16 tokens, stacked
    "scan": 1,                # the memory read + write over the frames
    "kpff": 1,                # key-pixel feature fusion
    "head": 1,                # the 1x1 classifier
    "seg_loss": 1,            # the fused objective
}


# ------------------------------------------------------------------------------------------------------------------------------------
# The tracer

@dataclass
class Arg:
    kind: str                      # "act" (an activation: passed through a tap), "param", "buf" (other tensors), "val" (non-tensors)
    value: Any                     # tensors: a detached clone taken when the call ran
    name: Optional[str] = None     # parameters and buffers: the model's name for it
    after: Optional[torch.Tensor] = None   # buffers: the value after the call (running statistics)


@dataclass
class Call:
    entry: str
    index: int
    args: List[Arg]
    outs: List[torch.Tensor] = field(default_factory=list)
    dout: Dict[int, torch.Tensor] = field(default_factory=dict)   # output index -> the gradient that arrived at it
    din: Dict[int, torch.Tensor] = field(default_factory=dict)    # arg index -> the gradient THIS call sent back to that input
    key: Optional[str] = None                                      # node name in wiring()


class _Tap(torch.autograd.Function):
    """Identity; its backward records the gradient that one consumer sends back to one of its inputs."""

    @staticmethod
    def forward(ctx, x, sink, slot):
        ctx.sink, ctx.slot = sink, slot
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        ctx.sink[ctx.slot] = g.detach().clone()
        return g, None, None


class StepTrace:
    """Wraps every ENTRY_POINTS function of gdkvm_amd.ops while installed.  Each wrapper records the call's tensor inputs (clones),
    parameters (by name, as they were when the call ran), running statistics before and after, flags and outputs; sends each
    activation input through a _Tap (the gradient this call alone returns to it) and hooks each output (the gradient arriving
    there).  No value changes: test_train_trace_gpu checks the traced step against an untraced one bit for bit."""

    def __init__(self, model: nn.Module):
        self.names = {id(p): n for n, p in model.named_parameters()}
        self.names.update({id(b): n for n, b in model.named_buffers()})
        self.calls: List[Call] = []

    def _wrap(self, entry, fn):
        def traced(*args, **kw):
            if kw:
                raise AssertionError(f"{entry} called with keywords {sorted(kw)}: the trace expects the positional layout")
            call = Call(entry, len(self.calls), [])
            self.calls.append(call)
            passed, bufs = [], []
            for a in args:
                if entry == "token_projections" and isinstance(a, (tuple, list)) and a and isinstance(a[0], nn.Module):
                    for m in a:                                      # the stacked layers: their weights and biases are the parameters
                        for p in (m.weight, m.bias):
                            call.args.append(Arg("param", p.detach().clone(), self.names[id(p)]))
                    passed.append(a)
                    continue
                if isinstance(a, torch.Tensor):
                    name = self.names.get(id(a))
                    if isinstance(a, nn.Parameter):
                        call.args.append(Arg("param", a.detach().clone(), name))
                    elif a.requires_grad and torch.is_grad_enabled():
                        call.args.append(Arg("act", a.detach().clone()))
                        a = _Tap.apply(a, call.din, len(call.args) - 1)
                    else:
                        call.args.append(Arg("buf", a.detach().clone(), name))
                        bufs.append((call.args[-1], a))
                else:
                    call.args.append(Arg("val", a))
                passed.append(a)
            out = fn(*passed)
            outs = out if isinstance(out, tuple) else (out,)
            for j, o in enumerate(outs):
                call.outs.append(o.detach().clone())
                if o.requires_grad:                                  # (an unused output -- the scan's final state -- may get None)
                    o.register_hook(lambda g, j=j: None if g is None else call.dout.__setitem__(j, g.detach().clone()))
            for rec, t in bufs:
                rec.after = t.detach().clone()
            return out
        return traced

    @contextlib.contextmanager
    def installed(self):
        from gdkvm_amd import ops
        mp = pytest.MonkeyPatch()
        try:
            for entry in ENTRY_POINTS:
                mp.setattr(ops, entry, self._wrap(entry, getattr(ops, entry)))
            yield self
        finally:
            mp.undo()


# ------------------------------------------------------------------------------------------------------------------------------------
# The wiring, from the architecture (oracle/model_plain.py), not from gdkvm_amd/model.py

FRAMES, TARGET = "<frames>", "<target>"


@dataclass
class Node:
    key: str
    entry: str
    inputs: Dict[int, tuple]       # arg position -> (source node | FRAMES | TARGET, output index, glue name)
    params: Dict[int, str]         # arg position -> parameter name
    statics: Dict[int, Any]        # arg position -> flag the call must have been made with
    alias: bool = False            # conv3x3_fork: output 1 IS input 0 (the block input, for the skip connection)


def wiring(cfg, B: int, T: int, H: int, W: int) -> List[Node]:
    """The training graph of GDKVM(cfg) at the default widths, in dataflow order, one Node per entry-point call:
    stem conv -> BN + ReLU + max-pool -> layer1 (two identity blocks) -> f4 -> layer2 (strided block, identity block) -> f8 -> layer3 -> f16
    -> the five stacked token projections -> scan -> KPFF(key, read-out, f16 tokens) -> up8 [upsample ; f8] -> up4 [upsample ; f4] -> head
    -> fused objective.  An identity block (stride 1, same width) takes its input through conv3x3_fork, whose second output is the skip;
    a strided block runs its 3x3 and 1x1 downsample convolutions as one conv_s2_block, the 1x1 branch through its own BatchNorm."""
    nodes: List[Node] = []
    eps = 1e-5

    def add(key, entry, inputs, params=None, statics=None, alias=False):
        nodes.append(Node(key, entry, {i: (s if len(s) == 3 else s + ("id",)) for i, s in inputs.items()}, params or {}, statics or {}, alias))
        return key

    def bn(key, src, relu, residual=None):
        ins = {0: src if isinstance(src, tuple) else (src, 0)}
        if residual is not None:
            ins[5] = residual
        return add(key, "bn_act", ins, {1: key + ".weight", 2: key + ".bias"}, {7: eps, 8: relu})

    def block(p, src, strided):
        if strided:
            c = add(p + ".conv1", "conv_s2_block", {0: (src, 0)}, {1: p + ".conv1.weight", 2: p + ".down.0.weight"})
            skip = (bn(p + ".down.1", (c, 1), False), 0)
        else:
            c = add(p + ".conv1", "conv3x3_fork", {0: (src, 0)}, {1: p + ".conv1.weight"}, alias=True)
            skip = (c, 1)
        y = bn(p + ".bn1", c, True)
        y = add(p + ".conv2", "conv3x3", {0: (y, 0)}, {1: p + ".conv2.weight"})
        return bn(p + ".bn2", y, True, residual=skip + ("id",))

    def up(p, src, skip):
        x = add(p + ".cat", "upsample_cat", {0: src, 1: (skip, 0)})
        for i in (0, 3):
            x = add(f"{p}.conv.{i}", "conv3x3", {0: (x, 0)}, {1: f"{p}.conv.{i}.weight"})
            x = bn(f"{p}.conv.{i + 1}", x, True)
        return x

    x = add("encoder.stem.0", "stem_conv", {0: (FRAMES, 0, "images")}, {1: "encoder.stem.0.weight"})
    x = add("encoder.stem.1", "bn_relu_pool", {0: (x, 0)}, {1: "encoder.stem.1.weight", 2: "encoder.stem.1.bias"}, {6: eps})
    f4 = block("encoder.layer1.1", block("encoder.layer1.0", x, False), False)
    f8 = block("encoder.layer2.1", block("encoder.layer2.0", f4, True), False)
    f16 = block("encoder.layer3.1", block("encoder.layer3.0", f8, True), False)
    projs = ("key_proj", "query_proj", "value_proj", "gate_proj", "decay_proj")          # stacked in this order: outputs 0 .. 4
    pr = add("key_proj", "token_projections", {0: (f16, 0, "rows")},
             {1 + 2 * i + j: f"{n}.{'weight' if j == 0 else 'bias'}" for i, n in enumerate(projs) for j in (0, 1)})
    sc = add("scan", "scan", {0: (pr, 1, "qk5"), 1: (pr, 0, "qk5"), 2: (pr, 2, "v5"), 3: (pr, 4, "alpha"), 4: (pr, 3, "beta")},
             statics={6: {"gated_linear": 0, "delta_parallel": 1, "delta_sequential": 2}[cfg.rule], 7: 3})
    kp = add("kpff", "kpff", {0: (pr, 0, "tok3"), 1: (sc, 0, "tok3"), 2: (f16, 0, "ntok3")},
             {3: "kpff.wa", 4: "kpff.ba", 5: "kpff.wl", 6: "kpff.wg"}, dict(zip((7, 8), feature_dims(H, W)[3])))
    y = up("decoder.up8", (kp, 0, "fmap"), f8)
    y = up("decoder.up4", (y, 0, "id"), f4)
    hd = add("decoder.head", "head", {0: (y, 0)}, {1: "decoder.head.weight", 2: "decoder.head.bias"})
    add("loss", "seg_loss", {0: (hd, 0), 1: (TARGET, 0, "labels")}, statics={2: 1.0, 3: 1.0})
    # (the order of independent nodes is free -- model_plain takes the downsample branch before conv2, the product after it): the
    # nodes in an order in which every node follows its sources
    done, order, pending = {FRAMES, TARGET}, [], list(nodes)
    while pending:
        for n in pending:
            if all(s[0] in done for s in n.inputs.values()):
                order.append(n); done.add(n.key); pending.remove(n)
                break
        else:
            raise AssertionError("wiring: a cycle")
    return order


def feature_dims(H: int, W: int):
    """Spatial sizes along the trunk: stem (stride 2), pool (4), stride 8, stride 16 (3x3 / stride 2 / pad 1 and friends)."""
    s2 = ((H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1)
    half = lambda hw: ((hw[0] - 1) // 2 + 1, (hw[1] - 1) // 2 + 1)
    s4 = half(s2)
    s8 = half(s4)
    return s2, s4, s8, half(s8)


def glue(name: str, t: torch.Tensor, cfg, B: int, T: int, H: int, W: int) -> torch.Tensor:
    """The framework reshapes between two calls, as the architecture defines them (tokens are pixels in row-major order, channels last)."""
    BT = B * T
    h, w = feature_dims(H, W)[3]
    N, Hh, Dk, Dv = h * w, cfg.heads, cfg.key_dim, cfg.value_dim
    wide = (lambda u: u.float()) if t.dtype == torch.bfloat16 else (lambda u: u)
    if name == "id":
        return t
    if name == "images":
        return t.reshape(BT, *t.shape[2:])
    if name == "labels":
        return t.reshape(BT, *t.shape[2:])
    if name == "rows":
        return t.permute(0, 2, 3, 1).reshape(BT * N, t.shape[1])
    if name == "ntok3":
        return t.permute(0, 2, 3, 1).reshape(BT, N, t.shape[1])
    if name == "qk5":
        return t.reshape(B, T, N, Hh, Dk)
    if name == "v5":
        return t.reshape(B, T, N, Hh, Dv)
    if name == "beta":                       # the write gate: one logit per token and head
        return wide(t).reshape(B, T, N, Hh)
    if name == "alpha":                      # the decay: one logit per frame and head, W_d mean_n(x) + b_d = mean_n(W_d x + b_d)
        return wide(t).reshape(BT, N, Hh).mean(1).reshape(B, T, Hh)
    if name == "tok3":
        return t.reshape(BT, N, -1)
    if name == "fmap":
        return t.reshape(BT, h, w, t.shape[-1]).permute(0, 3, 1, 2)
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------------------------------------------
# float64 references, one per entry point (differentiable: their VJPs are torch.autograd's)

def _w(t: torch.Tensor, bf16: bool) -> torch.Tensor:
    """A weight as the kernels read it: the fp32 master rounded to bf16 where the product packs / casts it (bf16=True)."""
    t = t.to(torch.float64)
    return t + (t.to(torch.bfloat16).to(torch.float64) - t).detach() if bf16 else t    # (straight through: the gradient is not rounded)


class _RoundGrad(torch.autograd.Function):
    """Identity forward; backward rounds the gradient to bf16 -- the stem's pooled backward gathers each pre-pool element's gradient from
    its windows and rounds the sum to bf16 (as the two-kernel form stored it) before the BatchNorm backward reduces it."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def _bn_train(x, g, b, eps):
    return F.batch_norm(x, None, None, g, b, True, 0.0, eps)


def reference(entry: str, a: list, bf16: bool = False, relu_mask: Optional[torch.Tensor] = None) -> tuple:
    """float64 outputs of one call from its positional arguments `a` (float64 tensors; labels as integers).
    bf16=True: the arithmetic of the bf16 training build made explicit -- weights rounded where the kernels' packs round them, the stem's
    max-pool choosing among the bf16-stored activations (csrc/bn.hip compares what it would have stored; ties -> first tap) and its
    gathered pre-pool gradient rounded to bf16, and the ReLU mask of a bn_act taken from the recorded output (relu_mask): a value within
    one rounding of zero may fall either side."""
    if entry == "stem_conv":
        return (F.conv2d(a[0], _w(a[1], bf16), None, 2, 3),)
    if entry == "bn_relu_pool":
        z = F.relu(_bn_train(a[0], a[1], a[2], a[6]))
        if bf16:
            z = _RoundGrad.apply(z + (z.to(torch.bfloat16).to(torch.float64) - z).detach())
        return (F.max_pool2d(z, 3, 2, 1),)
    if entry == "conv3x3":
        return (F.conv2d(a[0], _w(a[1], bf16), None, 1, 1),)
    if entry == "conv3x3_fork":
        return F.conv2d(a[0], _w(a[1], bf16), None, 1, 1), a[0] * 1.0
    if entry == "conv_s2_block":
        return F.conv2d(a[0], _w(a[1], bf16), None, 2, 1), F.conv2d(a[0], _w(a[2], bf16), None, 2, 0)
    if entry == "bn_act":
        y = _bn_train(a[0], a[1], a[2], a[7])
        if a[5] is not None:
            y = y + a[5]
        if a[8]:
            y = y * relu_mask.to(y.dtype) if relu_mask is not None else F.relu(y)
        return (y,)
    if entry == "upsample_cat":
        return (torch.cat([F.interpolate(a[0], size=a[1].shape[-2:], mode="bilinear", align_corners=False), a[1]], 1),)
    if entry == "token_projections":
        x = a[0]
        return tuple(x @ _w(wt, bf16).reshape(wt.shape[0], -1).T + bs for wt, bs in zip(a[1::2], a[2::2]))
    if entry == "scan":
        from oracle import torch_ref
        return torch_ref.scan(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7])
    if entry == "kpff":
        from oracle import torch_ref
        return (torch_ref.kpff(a[0], a[1], a[2], _w(a[3], bf16), a[4], _w(a[5], bf16), _w(a[6], bf16), a[7], a[8]),)
    if entry == "head":
        return (F.conv2d(a[0], a[1], a[2]),)
    if entry == "seg_loss":
        from oracle.model_plain import plain_objective
        z, tg = a[0], a[1]
        up = F.interpolate(z, size=tg.shape[-2:], mode="bilinear", align_corners=False)
        return (plain_objective(up.unsqueeze(0), tg.unsqueeze(0), a[2], a[3]),)
    raise KeyError(entry)


def vjp(outs: tuple, douts: Dict[int, torch.Tensor], leaves: List[torch.Tensor]) -> List[Optional[torch.Tensor]]:
    """sum_j <douts[j], d outs[j] / d leaf> for every leaf (float64); outputs without an arriving gradient contribute nothing."""
    ys, gs = [], []
    for j, o in enumerate(outs):
        if j in douts and o.requires_grad:
            ys.append(o)
            gs.append(douts[j].to(torch.float64).reshape(o.shape))
    if not ys:
        return [None] * len(leaves)
    return list(torch.autograd.grad(ys, leaves, gs, allow_unused=True))


def chain(cfg, sd: Dict[str, torch.Tensor], frames: torch.Tensor, target: torch.Tensor):
    """The per-call references chained along wiring() from the frames to the loss, all float64 on the CPU, call by call: forward node by
    node, then backward node by node in reverse, each node's VJP sent through the glue to the outputs that fed it -- the same per-call
    machinery the GPU test applies to a recorded step.  Returns (loss, {parameter name: gradient})."""
    B, T, C, H, W = frames.shape
    params = {k: v.detach().to(torch.float64) for k, v in sd.items() if v.is_floating_point() and "running_" not in k}
    srcs = {FRAMES: [frames.detach().to(torch.float64)], TARGET: [target.detach()]}
    nodes = wiring(cfg, B, T, H, W)
    saved = {}
    for n in nodes:
        feats = {i: srcs[s][j].detach().requires_grad_(s not in (FRAMES, TARGET)) for i, (s, j, g) in n.inputs.items()}
        args = _arg_list(n, {i: glue(n.inputs[i][2], f, cfg, B, T, H, W) for i, f in feats.items()},
                         {i: params[p].clone().requires_grad_() for i, p in n.params.items()}, cfg, H, W)
        outs = reference(n.entry, args, bf16=False)
        srcs[n.key] = [o.detach() for o in outs]
        saved[n.key] = (feats, args, outs)
    grads_out = {n.key: {} for n in nodes}
    grads_out["loss"] = {0: torch.ones((), dtype=torch.float64)}
    pgrad: Dict[str, torch.Tensor] = {}
    for n in reversed(nodes):
        feats, args, outs = saved[n.key]
        leaf_pos = [i for i in feats if n.inputs[i][0] not in (FRAMES, TARGET)] + list(n.params)
        leaves = [feats[i] if i in feats else args[i] for i in leaf_pos]
        gs = vjp(outs, grads_out[n.key], leaves)
        for i, g in zip(leaf_pos, gs):
            if g is None:
                continue
            if i in n.params:
                pgrad[n.params[i]] = pgrad.get(n.params[i], 0) + g
            else:
                s, j, _ = n.inputs[i]
                acc = grads_out[s]
                acc[j] = acc[j] + g if j in acc else g
    return srcs["loss"][0], pgrad


def _arg_list(n: Node, feats: Dict[int, torch.Tensor], params: Dict[int, torch.Tensor], cfg, H: int, W: int) -> list:
    """The positional argument list of a wiring node (bookkeeping arguments -- running statistics, momentum, state -- as None / 0)."""
    size = {"stem_conv": 2, "bn_relu_pool": 7, "conv3x3_fork": 2, "conv3x3": 2, "conv_s2_block": 3, "bn_act": 9, "upsample_cat": 2,
            "token_projections": 11, "scan": 8, "kpff": 9, "head": 3, "seg_loss": 4}[n.entry]
    a: list = [None] * size
    for i, t in feats.items():
        a[i] = t
    for i, t in params.items():
        a[i] = t
    for i, v in n.statics.items():
        a[i] = v
    return a
