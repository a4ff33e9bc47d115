"""Poisoned, guarded outputs and workspaces for every kernel entry of gdkvm_amd.ops (plain Python, importable without a GPU).

`poisoned(byte)` is a context manager.  While it is active

  * the name `torch` inside gdkvm_amd.ops (and any further module given) is a proxy that forwards everything to the real module except
    `empty`, `empty_like` and `empty_strided`: those hand back a tensor of the same shape, strides, dtype and device that sits `guard`
    bytes inside a flat buffer filled with `byte`, with `guard` bytes of the same pattern behind it.  The global torch module is untouched;
  * ops._workspace / ops._grown_workspace ask the real size query (ops._bytes) and hand back `big[guard:guard + need]` of a `byte`-filled
    `big`: exactly the bytes the query asks for (at least the wrapper's floor), never the grown buffer of an earlier, larger call;
  * ops._call is wrapped by a pass-through that notes, per launch, how many buffers had been handed out before it (so that a test can say
    which outputs a refused launch should have left alone);
  * every buffer handed out is recorded (`Poisoned.records`).

`check_guards()` asserts that no byte before or after any payload changed, `unwritten(t)` is the mask of elements that still hold the
pattern.  Every patched name is restored on exit, also after an exception.

The second half of the file is ENTRIES: one row per workspace-taking entry point, each with the callable that runs the op through its
`ops` wrapper at the smallest shapes where its scratch logic has more than one case, and the existing reference check the row applies."""
import contextlib
import inspect
import os
import re
from dataclasses import dataclass, field
from types import SimpleNamespace as NS
from typing import Callable, Optional

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096
PATTERNS = (0x00, 0xFF, 0x5A)
_INT_OF = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_PATCHED = ("empty", "empty_like", "empty_strided")


def pattern_value(byte: int, itemsize: int) -> int:
    """The integer an element of `itemsize` bytes holds when every byte of it is `byte` (signed for 2, 4 and 8 bytes: what a view as
    int16 / int32 / int64 reads; uint8 for one byte)."""
    v = int.from_bytes(bytes([byte]) * itemsize, "little", signed=False)
    if itemsize > 1 and v >= 1 << (8 * itemsize - 1):
        v -= 1 << (8 * itemsize)
    return v


def bits(t: torch.Tensor) -> torch.Tensor:
    """t's elements as integers of the same width (bool: as uint8): what bit equality and the poison test compare."""
    if t.dtype == torch.bool:
        return t.to(torch.uint8)
    return t.view(_INT_OF[t.element_size()])


def bit_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """torch.equal on the bits: NaNs with equal payloads are equal, +0 and -0 are not."""
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


@dataclass
class Record:
    kind: str                       # "output" | "workspace"
    name: str                       # size-query name, or file:line function of the allocation site
    flat: torch.Tensor              # uint8 [guard + nbytes + guard]
    lo: int                         # payload range inside flat, in bytes
    hi: int
    tensor: Optional[torch.Tensor] = None     # the tensor handed out
    need: int = 0                   # workspaces: what the size query (and floor) asked for
    query: int = 0                  # workspaces: what the size query alone returned
    seq: int = 0                    # position in Poisoned.records


class _TorchProxy:
    """`torch` as a module sees it under poisoned(): every attribute is the real module's, but for the three allocators."""

    def __init__(self, owner: "Poisoned"):
        object.__setattr__(self, "_owner", owner)

    def __getattr__(self, name):
        if name in _PATCHED:
            return getattr(object.__getattribute__(self, "_owner"), "_" + name)
        return getattr(torch, name)

    def __setattr__(self, name, value):
        raise AttributeError("the torch proxy of tests/poisoned_buffers.py is read-only")


def _site() -> str:
    """file:line function of the first frame outside this file."""
    here = os.path.abspath(__file__)
    f = inspect.currentframe()
    while f is not None and os.path.abspath(f.f_code.co_filename) == here:
        f = f.f_back
    if f is None:
        return "?"
    return f"{os.path.basename(f.f_code.co_filename)}:{f.f_lineno} {f.f_code.co_name}"


class Poisoned:
    def __init__(self, byte: int, guard: int = GUARD, grown: str = "exact", modules=(), short: Optional[str] = None, short_by: int = 16):
        if not 0 <= byte <= 255 or guard <= 0 or guard % 16 or grown not in ("exact", "real"):
            raise ValueError("poisoned(byte in 0..255, guard a positive multiple of 16, grown 'exact' or 'real')")
        self.byte, self.guard, self.grown = byte, guard, grown
        self.short, self.short_by = short, short_by
        self.modules = tuple(modules)
        self.records = []
        self.calls = []             # (entry name, len(records) before the launch, "ok" | the exception)
        self._saved = []

    # ---------------------------------------------------------------------------------------------------------------- allocation
    def _flat(self, nbytes: int, device) -> torch.Tensor:
        return torch.full((self.guard + nbytes + self.guard,), self.byte, dtype=torch.uint8, device=device)

    def _like(self, real: torch.Tensor) -> torch.Tensor:
        """A poisoned, guarded stand-in for `real` (a fresh tensor of the real allocator): same shape, strides, dtype, device."""
        if real.numel() == 0 or real.is_sparse or real.layout != torch.strided or (real.device.type == "cpu" and real.is_pinned()):
            return real
        es = real.element_size()
        extent = 1 + sum((n - 1) * s for n, s in zip(real.shape, real.stride()))          # elements from the first to the last one
        nbytes = extent * es
        flat = self._flat(nbytes, real.device)
        t = flat.view(real.dtype).as_strided(tuple(real.shape), tuple(real.stride()), self.guard // es)
        if real.requires_grad:
            t.requires_grad_()
        rec = Record("output", _site(), flat, self.guard, self.guard + nbytes, t, seq=len(self.records))
        self.records.append(rec)
        return t

    def _empty(self, *a, **kw):
        return self._like(torch.empty(*a, **kw))

    def _empty_like(self, *a, **kw):
        return self._like(torch.empty_like(*a, **kw))

    def _empty_strided(self, *a, **kw):
        return self._like(torch.empty_strided(*a, **kw))

    # ---------------------------------------------------------------------------------------------------------------- workspaces
    def _ws(self, name: str, dev, need: int, query: int) -> torch.Tensor:
        if need == 0:
            return torch.empty(0, dtype=torch.uint8, device=dev)                        # (what the wrapper passes as NULL, 0)
        big = self._flat(need, dev)
        give = need - self.short_by if (self.short == name and query > 16) else need
        t = big[self.guard:self.guard + give]
        self.records.append(Record("workspace", name, big, self.guard, self.guard + need, t, need, query, len(self.records)))
        return t

    def _workspace(self, name: str, dev, *dims, floor: int = 0) -> torch.Tensor:
        query = self._ops._bytes(name, dev, *dims)
        return self._ws(name, dev, max(floor, query), query)

    def _grown_workspace(self, name: str, dev, *dims) -> torch.Tensor:
        query = self._ops._bytes(name, dev, *dims)
        need = max(16, query)
        if self.grown == "exact":
            return self._ws(name, dev, need, query)
        ws = self._real_grown(name, dev, *dims)                                         # the product's own, grown buffer ...
        if ws.numel() > need:
            ws[need:] = self.byte                                                      # ... stale partials past this call's share poisoned
        self.records.append(Record("grown", name, ws, 0, ws.numel(), ws, need, query, len(self.records)))
        return ws

    def _call(self, name: str, dev, *args) -> None:
        at = len(self.records)
        try:
            self._real_call(name, dev, *args)
        except Exception as e:
            self.calls.append((name, at, e))
            raise
        self.calls.append((name, at, "ok"))

    # ---------------------------------------------------------------------------------------------------------------- context
    def _patch(self, obj, name, value):
        self._saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def __enter__(self):
        from gdkvm_amd import ops
        self._ops = ops
        try:
            proxy = _TorchProxy(self)
            for mod in (ops,) + self.modules:
                if getattr(mod, "torch", None) is not torch:
                    raise RuntimeError(f"{mod.__name__}.torch is not the torch module (already patched?)")
                self._patch(mod, "torch", proxy)
            self._real_grown, self._real_call = ops._grown_workspace, ops._call
            self._patch(ops, "_workspace", self._workspace)
            self._patch(ops, "_grown_workspace", self._grown_workspace)
            self._patch(ops, "_call", self._call)
        except BaseException:
            self._restore()
            raise
        return self

    def _restore(self):
        while self._saved:
            obj, name, old = self._saved.pop()
            setattr(obj, name, old)

    def __exit__(self, *exc):
        self._restore()
        return False

    # ---------------------------------------------------------------------------------------------------------------- checks
    def outputs(self, since: int = 0):
        return [r for r in self.records[since:] if r.kind == "output"]

    def workspaces(self, name: Optional[str] = None):
        return [r for r in self.records if r.kind in ("workspace", "grown") and (name is None or r.name == name)]

    def check_guards(self) -> None:
        """Every byte before and after every payload still holds the pattern (synchronises: the comparison reads the buffers)."""
        for r in self.records:
            if r.kind == "grown":
                tail = r.flat[r.need:]
                bad = (tail != self.byte).nonzero()
                assert bad.numel() == 0, (f"workspace {r.name} (record {r.seq}): byte {r.need + int(bad[0])} of the grown buffer, past the "
                                          f"{r.need} bytes this call may use, was written")
                continue
            for what, part, base in (("before", r.flat[:r.lo], -r.lo), ("after", r.flat[r.hi:], 0)):
                bad = (part != self.byte).nonzero()
                assert bad.numel() == 0, (f"{r.kind} {r.name} (record {r.seq}, payload {r.hi - r.lo} bytes): {bad.numel()} guard byte(s) "
                                          f"{what} it were written, the first at offset {base + int(bad[0])} from the payload's "
                                          f"{'start' if what == 'before' else 'end'}")

    def unwritten(self, t: torch.Tensor) -> torch.Tensor:
        """bool mask, shaped like t: the elements whose every byte still equals the pattern."""
        return bits(t) == pattern_value(self.byte, 1 if t.dtype == torch.bool else t.element_size())

    def payload_intact(self, r: Record) -> bool:
        """Whether the whole payload of a record still holds the pattern (zero-size workspaces: the 16 floor bytes; refused launches)."""
        return bool((r.flat[r.lo:r.hi] == self.byte).all())


def poisoned(byte: int, guard: int = GUARD, **kw) -> Poisoned:
    return Poisoned(byte, guard, **kw)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Census: what include/gdkvm.h declares and what the wrappers name
def declared_queries(header=os.path.join(ROOT, "include", "gdkvm.h")):
    """Every size query the header DECLARES (`size_t gdkvm_..._workspace_bytes(`), in order."""
    return re.findall(r"^\s*(?:GDKVM_API\s+)?size_t\s+(gdkvm_\w+_workspace_bytes)\s*\(", open(header).read(), re.M)


def named_queries(pkg=os.path.join(ROOT, "gdkvm_amd")):
    """{query name: [file:line]} for every _workspace( / _grown_workspace( call site of the package.  A name built at run time
    (`name + "_workspace_bytes"`, `entry + "_workspace_bytes"`) is expanded through DYNAMIC_SITES; an unknown one is reported as it stands."""
    out = {}
    for fn in sorted(os.listdir(pkg)):
        if not fn.endswith(".py"):
            continue
        for no, line in enumerate(open(os.path.join(pkg, fn)), 1):
            if re.match(r"\s*def ", line):
                continue
            for m in re.finditer(r"\b_(?:grown_)?workspace\(\s*([^,)]+)", line):
                arg = m.group(1).strip()
                lit = re.fullmatch(r"[\"'](\w+)[\"']", arg)
                names = [lit.group(1)] if lit else DYNAMIC_SITES.get(arg, [arg])
                for n in names:
                    out.setdefault(n, []).append(f"{fn}:{no}")
    return out


# run-time names of two call sites: ops.wgrad (`name` is one of two entries) and ops._surface_distance (`entry` is one of two)
DYNAMIC_SITES = {
    'name + "_workspace_bytes"': ["gdkvm_gemm_tn_workspace_bytes", "gdkvm_gemm_tn_colsum_workspace_bytes"],
    'entry + "_workspace_bytes"': ["gdkvm_surface_distance_workspace_bytes", "gdkvm_surface_distance_mm_workspace_bytes"],
}


# ---------------------------------------------------------------------------------------------------------------------------------------
# ENTRIES: one row per workspace-taking entry point.  `run(ops, case)` builds the case's inputs (seeded: the same on every call), runs the op
# through its ops wrapper and returns {name: output tensor}; `check(ops, case, outs)` applies the reference check of the entry's existing test
# (named in `reference`), importing that test's helper where it has one.  Everything a row needs from a GPU test module is imported inside
# its functions: this file stays importable without a GPU.
@dataclass
class Row:
    name: str
    queries: tuple                  # the size queries the row's wrappers ask
    cases: list
    run: Callable
    check: Callable
    reference: str
    note: str = ""
    ids: list = field(default_factory=list)

    def __post_init__(self):
        self.ids = ["-".join(str(x).replace("torch.", "") for x in c) if isinstance(c, tuple) else str(c) for c in self.cases]


CL = dict(memory_format=torch.channels_last)
BF16, F32 = torch.bfloat16, torch.float32
DT = {"bf16": BF16, "fp32": F32}


def _cuda(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t.to(dtype) if dtype is not None else t


# ---- BN and head ---------------------------------------------------------------------------------------------------------------------------
BN_SHAPES = [(2, 8, 1, 2), (5, 24, 9, 4), (16, 64, 56, 56)]


def _bn_inputs(case):
    shape, mode = case
    torch.manual_seed(sum(shape) + len(mode))
    x = (3.0 + 2.0 * torch.randn(shape, device="cuda")).to(BF16).contiguous(**CL)
    res = torch.randn(shape, device="cuda").to(BF16).contiguous(**CL) if "res" in mode else None
    w = torch.rand(shape[1], device="cuda") + 0.5
    b = 0.3 * torch.randn(shape[1], device="cuda")
    dy = torch.randn(shape, device="cuda").to(BF16).contiguous(**CL)
    return x, res, w, b, dy


def _bn_act_run(ops, case):
    x, res, w, b, dy = _bn_inputs(case)
    rm, rv = torch.zeros(x.shape[1], device="cuda"), torch.ones(x.shape[1], device="cuda")
    xg, wg, bg = x.clone(**CL).requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    rg = None if res is None else res.clone(**CL).requires_grad_(True)
    y = ops.bn_act(xg, wg, bg, rm, rv, rg, 0.1, 1e-5, True)
    y.backward(dy)
    out = dict(y=y.detach(), dx=xg.grad, dgamma=wg.grad, dbeta=bg.grad, rm=rm, rv=rv)
    if rg is not None:
        out["dres"] = rg.grad
    return out


def _bn_act_check(ops, case, o):
    from tests.test_train_side_gpu import _bn_act_close, _reference
    x, res, w, b, dy = _bn_inputs(case)
    _bn_act_close(BF16, o["y"], o["rm"], o["rv"], o["dx"], o["dgamma"], o["dbeta"], o.get("dres"), _reference(x, w, b, res, True, dy, o["y"] > 0))


def _bn_pool_inputs(shape):
    torch.manual_seed(sum(shape))
    n, c, hh, ww = shape
    x = (torch.randn(shape, device="cuda") * 4).round().div(4).bfloat16().contiguous(**CL)
    g, b = torch.rand(c, device="cuda") + 0.5, torch.randn(c, device="cuda") * 0.2
    dy = torch.randn(n, c, (hh - 1) // 2 + 1, (ww - 1) // 2 + 1, device="cuda").bfloat16().contiguous(**CL)
    return x, g, b, dy


def _bn_pool_run(ops, shape, fused=True):
    x, g, b, dy = _bn_pool_inputs(shape)
    c = shape[1]
    xa, ga, ba = x.clone(**CL).requires_grad_(True), g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    rm, rv = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
    y = ops.bn_relu_pool(xa, ga, ba, rm, rv, 0.1, 1e-5) if fused else ops.maxpool3x3s2(ops.bn_act(xa, ga, ba, rm, rv, None, 0.1, 1e-5, True))
    y.backward(dy)
    return dict(y=y.detach(), dx=xa.grad, dgamma=ga.grad, dbeta=ba.grad, rm=rm, rv=rv)


def _bn_pool_check(ops, shape, o):
    """test_batchnorm_relu_maxpool_as_one_op: against maxpool3x3s2(bn_act(x)) -- run by the caller OUTSIDE any poisoned block."""
    a = _bn_pool_run(ops, shape, fused=False)
    assert torch.equal(a["y"], o["y"]) and torch.equal(a["rm"], o["rm"]) and torch.equal(a["rv"], o["rv"])
    for k in ("dgamma", "dbeta"):
        assert (a[k] - o[k]).abs().max() <= 1e-5 * max(1.0, a[k].abs().max().item())
    d = (a["dx"].float() - o["dx"].float()).abs()
    assert d.max() <= 2.0 ** -7 * max(1.0, a["dx"].float().abs().max().item()) and (d > 0).float().mean() <= 1e-2
    if 256 % (shape[1] // 8):
        assert torch.equal(a["dx"], o["dx"]) and torch.equal(a["dgamma"], o["dgamma"])


def _head_inputs(case):
    n, c, hh, ww, ncls, dtype = case
    torch.manual_seed(sum(case[:5]))
    x = torch.randn(n, c, hh, ww, device="cuda").to(dtype).contiguous(**CL)
    conv = torch.nn.Conv2d(c, ncls, 1).cuda()
    gz = torch.randn(n, ncls, hh, ww, device="cuda").to(dtype)
    return x, conv.weight.detach(), conv.bias.detach(), gz


def _head_run(ops, case):
    x, w, b, gz = _head_inputs(case)
    x, w, b = x.requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    z = ops.head(x, w, b)
    z.backward(gz)
    return dict(z=z.detach(), dx=x.grad, dw=w.grad, db=b.grad)


def _head_check(ops, case, o):
    import torch.nn.functional as Fn
    x, w, b, gz = _head_inputs(case)
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    z64 = Fn.conv2d(x64, w64, b64)
    z64.backward(gz.double())
    from tests.test_train_side_gpu import _head_close
    assert o["z"].is_contiguous() and o["z"].dtype == case[5]
    _head_close(case[5], o["z"], o["dx"], o["dw"], o["db"], z64, x64.grad, w64.grad, b64.grad)


# ---- split-K products ------------------------------------------------------------------------------------------------------------------------
def _wgrad_inputs(case):
    tokens, dtype, _ = case
    g = torch.Generator(device="cuda").manual_seed(tokens)
    x = torch.randn(tokens, 64, device="cuda", generator=g).to(dtype)
    dy = torch.randn(tokens, 40, device="cuda", generator=g).to(dtype)
    return dy, x


def _wgrad_run(ops, case):
    dy, x = _wgrad_inputs(case)
    if case[2]:
        dw, db = ops.wgrad(dy, x, colsum=True)
        return dict(dw=dw, db=db)
    return dict(dw=ops.wgrad(dy, x))


def _wgrad_check(ops, case, o):
    from tests.test_train_side_gpu import _colsum_close, _wgrad_close
    dy, x = _wgrad_inputs(case)
    _wgrad_close(o["dw"], dy.double().t() @ x.double(), case[0])
    if case[2]:
        _colsum_close(o["db"], dy.double().cpu().sum(0), case[0])


WG_SMALLEST, WG_LARGEST, WG_TINY = (129, 128, 128, 14, 14), (400, 64, 64, 28, 28), (5, 64, 64, 3, 2)
_ref_cache = {}


def _conv3_inputs(shape):
    """(x, dy, fp64 reference): the cached operands of tests/test_wgrad_tiles_gpu.py for its own cases, made the same way for the tiny one."""
    from tests import test_wgrad_tiles_gpu as W
    if shape in W.WG_CASES:
        return W._wg_inputs(shape)
    if shape not in _ref_cache:
        n, c, k, h, w = shape
        gen = torch.Generator(device="cuda").manual_seed(sum(shape))
        x, dy = W._randn_bf16((n, c, h, w), gen, **CL), W._randn_bf16((n, k, h, w), gen, **CL)
        _ref_cache[shape] = (x, dy, W.ref_wgrad(x, dy, 3, 1, 1))
    return _ref_cache[shape]


def _conv3_run(ops, case):
    x, dy, _ = _conv3_inputs(case[0])
    return dict(dw=ops.conv3x3_wgrad(x, dy, channels_last=case[1]))


def _conv3_check(ops, case, o):
    from tests.test_train_side_gpu import conv3x3_wgrad_bound
    (n, c, k, h, w), channels_last = case
    ref = _conv3_inputs(case[0])[2]
    dw = o["dw"]
    assert dw.dtype == F32 and dw.shape == ref.shape and (dw.is_contiguous(**CL) if channels_last else dw.is_contiguous())
    assert (dw.double() - ref).abs().max().item() <= conv3x3_wgrad_bound(ref, n * h * w)


STRIDED_CASES = [(2, 64, 64, 12, 10, 3, 1, 1), (3, 128, 40, 9, 9, 1, 2, 0), (1, 64, 72, 16, 16, 5, 2, 2), (2, 64, 64, 8, 8, 3, 3, 0)]   # = STRIDED_WINDOW_CASES


def _strided_inputs(shape):
    if shape not in _ref_cache:
        from tests.test_wgrad_tiles_gpu import ref_wgrad
        n, c, k, hh, ww, r, stride, pad = shape
        gen = torch.Generator(device="cuda").manual_seed(sum(shape))
        ho, wo = (hh + 2 * pad - r) // stride + 1, (ww + 2 * pad - r) // stride + 1
        x = torch.randn(n, c, hh, ww, device="cuda", generator=gen).bfloat16().contiguous(**CL)
        gy = torch.randn(n, k, ho, wo, device="cuda", generator=gen).bfloat16().contiguous(**CL)
        _ref_cache[shape] = (x, gy, ref_wgrad(x, gy, r, stride, pad))
    return _ref_cache[shape]


def _strided_run(ops, case):
    shape, channels_last = case
    n, c, k, hh, ww, r, stride, pad = shape
    x, gy, _ = _strided_inputs(shape)
    like = torch.zeros(k, c, r, r, device="cuda")
    if channels_last:
        like = like.contiguous(**CL)
    return dict(dw=ops.conv_wgrad_strided(x, gy, like, stride, pad), like=like)


def _strided_check(ops, case, o):
    from tests.test_train_side_gpu import _strided_wgrad_close
    _strided_wgrad_close(o["dw"], _strided_inputs(case[0])[2], o["like"])


def _stem_inputs(case):
    n, c, hh, ww = case
    torch.manual_seed(sum(case))
    x = torch.randn(n, c, hh, ww, device="cuda").bfloat16()
    w = torch.randn(64, c, 7, 7, device="cuda") / (49 * c) ** 0.5
    gy = torch.randn(n, 64, hh // 2, ww // 2, device="cuda").bfloat16().contiguous(**CL)
    return x, w, gy


def _stem_run(ops, case):
    x, w, gy = _stem_inputs(case)
    w = torch.nn.Parameter(w)
    y = ops.stem_conv(x, w)
    (dw,) = torch.autograd.grad(y, w, gy)
    return dict(y=y.detach(), dw=dw)


def _stem_check(ops, case, o):
    import torch.nn.functional as Fn
    n, c, hh, ww = case
    x, w, gy = _stem_inputs(case)
    w64 = w.bfloat16().double().requires_grad_()
    ref = Fn.conv2d(x.double(), w64, None, 2, 3)
    from tests.test_train_side_gpu import _stem_forward_close, _stem_wgrad_close
    _stem_forward_close(o["y"], ref)
    (dref,) = torch.autograd.grad(ref, w64, gy.double())
    _stem_wgrad_close(o["dw"], dref, w, n, hh, ww)


EMBED_GEOMS = [(4, 64, 64, 4, 4, 1024, 4), (5, 120, 88, 7, 6, 64, 4), (512, 112, 112, 7, 7, 256, 2)]
_embed_cache = {}


def _embed_inputs(case):
    if case not in _embed_cache:
        from tests.test_feedback_train_gpu import _masks, _wgrad_ref
        (F_, H, W, h, w, C, ncls), dtype = case
        m = _masks(F_, H, W, ncls, seed=F_ + H + C)
        dv = torch.randn(F_, h * w, C, generator=torch.Generator().manual_seed(C + F_)).to(dtype)
        _embed_cache[case] = (m.cuda(), dv.cuda(), _wgrad_ref(m, dv, h, w))
    return _embed_cache[case]


def _embed_run(ops, case):
    m, dv, _ = _embed_inputs(case)
    return dict(dw=ops.mask_embed_wgrad(m, dv, case[0][3], case[0][4]))


def _embed_check(ops, case, o):
    ref = _embed_inputs(case)[2]
    assert o["dw"].dtype == F32 and o["dw"].shape == (case[0][5],)
    assert np.abs(o["dw"].cpu().double().numpy() - ref).max() / np.abs(ref).max() <= 1e-5


# ---- KPFF and losses ---------------------------------------------------------------------------------------------------------------------------
KPFF_ALIGNED, KPFF_RAGGED = (5, 3, 32, 32, 32), (5, 3, 16, 48, 80)            # kpff_forms.CASES["h"]; kpff_forms.SAVES_EXACT[0]
KPFF_CASES = [(s, d) for s in (KPFF_ALIGNED, KPFF_RAGGED) for d in ("bf16", "fp32")]


def _kpff_arrays(shape):
    from tests import kpff_forms as kf
    from tests.util import make_kpff_inputs
    h, w, ck, cv, cp = shape
    return make_kpff_inputs(kf.SMALL_BT, h, w, ck, cv, cp, seed=sum(shape))


def _kpff_oracle(case):
    """c_oracle.kpff on the operands as the case's arm reads them, and the bound of the arm's test in tests/test_kpff_argmax_gpu.py."""
    from oracle import c_oracle
    from oracle import gdkvm_oracle as O
    shape, io = case
    h, w = shape[:2]
    L, G, P, Wa, ba, Wl, Wg = _kpff_arrays(shape)
    aligned = all(c % 32 == 0 for c in shape[2:])
    if io == "bf16":
        L, G, P = (O.to_bf16_f32(x) for x in (L, G, P))
        if aligned:                                           # test_kpff_bf16_mfma_arm: the weights are packed as bf16 too
            Wa, Wl, Wg = (O.to_bf16_f32(x) for x in (Wa, Wl, Wg))
    Fo = c_oracle.kpff(L, G, P, Wa, ba, Wl, Wg, h, w)
    if io == "bf16":
        return Fo, (4e-3 if aligned else 1e-4) + np.abs(Fo) * 2.0 ** -8
    return Fo, np.full_like(Fo, 3e-5 if aligned else 1e-4)    # test_kpff_fp32_on_bf16_splits / test_kpff_fp32


def _kpff_fwd_run(ops, case):
    shape, io = case
    arrs = _kpff_arrays(shape)
    feats = [_cuda(x, DT[io]) for x in arrs[:3]]
    return dict(F=ops.kpff_fwd(*feats, *(_cuda(x) for x in arrs[3:]), shape[0], shape[1]))


def _kpff_fwd_check(ops, case, o):
    Fo, lim = _kpff_oracle(case)
    assert np.all(np.abs(o["F"].float().cpu().numpy() - Fo) <= lim)


_KPFF_NAMES = "L G P Wa ba Wl Wg".split()


def _kpff_train_run(ops, case):
    shape, io = case
    h, w, ck, cv, cp = shape
    arrs = _kpff_arrays(shape)
    gs = [(_cuda(x, DT[io]) if i < 3 else _cuda(x)).requires_grad_() for i, x in enumerate(arrs)]
    dF = torch.randn(arrs[0].shape[0], h * w, cp, generator=torch.Generator().manual_seed(50)).to(DT[io]).cuda()
    f = ops.kpff(*gs, h, w)
    f.backward(dF)
    out = {"d" + n: t.grad for n, t in zip(_KPFF_NAMES, gs)}
    out["F"] = f.detach()
    return out


def _kpff_train_check(ops, case, o):
    """F as kpff_fwd's; gradients with the bounds of test_whole_backward_in_the_large_forms (tests/test_kpff_train_forms_gpu.py)."""
    from oracle import torch_ref as TR
    shape, io = case
    h, w, ck, cv, cp = shape
    _kpff_fwd_check(ops, case, o)
    arrs = [torch.from_numpy(x) for x in _kpff_arrays(shape)]
    aligned = all(c % 32 == 0 for c in shape[2:])
    rnd = (lambda i, x: x.bfloat16() if (i < 3 or (aligned and i != 4)) else x) if io == "bf16" else (lambda i, x: x)
    ts = [rnd(i, x).double().requires_grad_() for i, x in enumerate(arrs)]
    dF = torch.randn(arrs[0].shape[0], h * w, cp, generator=torch.Generator().manual_seed(50)).to(DT[io])
    (TR.kpff(*ts, h, w) * dF.double()).sum().backward()
    for name, t in zip(_KPFF_NAMES, ts):
        err, scale = (o["d" + name].double().cpu() - t.grad).abs(), t.grad.abs().max().item()
        if io == "bf16":
            assert err.max().item() <= 0.03 * scale + 1e-2 and err.mean().item() <= 4e-3 * scale + 1e-3, (name, err.max().item(), scale)
        else:
            assert err.max().item() <= 2e-4 * max(1.0, scale), (name, err.max().item(), scale)


LOSS_CASES = [((2, 3, 7, 5, 30, 17), torch.int64, False), ((2, 2, 9, 9, 5, 6), torch.uint8, False), ((2, 3, 7, 5, 30, 17), torch.uint8, True)]
LOSS_CASES = [c + (d,) for c in LOSS_CASES for d in (F32, BF16)]


def _loss_run(boundary):
    def run(ops, case):
        from tests.test_boundary_loss_gpu import _loss_case
        shape, tdt, unlabelled, dtype = case
        z, t, _, _ = _loss_case(shape, unlabelled)
        za = z.to(dtype).cuda().requires_grad_(True)
        tg = t.cuda().to(tdt)
        if boundary:
            loss, terms = ops.seg_loss_boundary(za, tg, 0.7, 1.0, 0.05, terms=True)
        else:
            loss, terms = ops.seg_loss(za, tg, 0.7, 1.0), None
        (3.0 * loss).backward()
        out = dict(loss=loss.detach(), dz=za.grad)
        if terms is not None:
            out["terms"] = terms
        return out
    return run


def _loss_check(boundary):
    def check(ops, case, o):
        from tests import boundary_reference as B
        from tests.test_boundary_loss_gpu import _loss_case
        shape, tdt, unlabelled, dtype = case
        z, t, sd2, _ = _loss_case(shape, unlabelled)
        zb = z.to(dtype).double().requires_grad_(True)
        ref, ce, dice, lb = B.objective_lowres(zb, t, 0.7, 1.0, 0.05 if boundary else 0.0, None, sd2)
        (3.0 * ref).backward()
        assert abs(o["loss"].item() - ref.item()) <= 1e-5 * max(1.0, abs(ref.item()))
        if boundary:
            tm = o["terms"]
            assert abs(tm[3].item() - lb.item()) <= 1e-5 * max(1.0, abs(lb.item())) and abs(tm[1].item() - ce.item()) <= 1e-5 * max(1.0, abs(ce.item()))
            assert abs(tm[2].item() - dice.item()) <= 1e-5 and tm[0].item() == o["loss"].item()
        scale = zb.grad.abs().max().item()
        assert (o["dz"].double().cpu() - zb.grad).abs().max().item() <= (2.0 ** -7 if dtype == BF16 else 1e-4) * scale
    return check


SD_SHAPES = [(256, 312), (256, 313)]


def _sd_labels(hw):
    from tests.test_boundary_loss_gpu import _labels
    return _labels(1, 2, hw[0], hw[1], 30)


def _sd_run(ops, hw):
    return dict(sd2=ops.signed_distance(_cuda(_sd_labels(hw)), 2))


def _sd_check(ops, hw, o):
    from tests import boundary_reference as B
    if hw not in _ref_cache:
        _ref_cache[hw] = B.sd2_reference(_sd_labels(hw), 2)
    assert o["sd2"].dtype == torch.int32 and np.array_equal(o["sd2"].cpu().numpy().astype(np.int64), _ref_cache[hw])


# ---- scan family -------------------------------------------------------------------------------------------------------------------------------
SCAN_FWD_CASES = [(rule, flags, d) for rule in (0, 1, 2) for flags in (0, 3) for d in ("fp32", "bf16")]
SCAN_FWD_SUB = [(N, Dk, Dv) for N in (7, 64, 65, 130) for Dk in (16, 20, 64, 72) for Dv in (16, 48)]
SCAN_BT = (2, 3)


def _scan_inputs(B, T, N, Hh, Dk, Dv, flags, bf16, seed):
    from oracle import gdkvm_oracle as O
    from tests.util import make_scan_inputs
    q, k, v, a, b = make_scan_inputs(B, T, N, Hh, Dk, Dv, seed=seed, normalized=not flags, logits=bool(flags), corr=0.5)
    s0 = (0.1 * np.random.default_rng(seed + 1).standard_normal((B, Hh, Dk, Dv))).astype(np.float32)
    if bf16:
        q, k, v = (O.to_bf16_f32(x) for x in (q, k, v))
    return q, k, v, a, b, s0


def _scan_fwd_run(ops, case):
    rule, flags, d = case
    out = {}
    for N, Dk, Dv in SCAN_FWD_SUB:
        q, k, v, a, b, s0 = _scan_inputs(*SCAN_BT, N, 1, Dk, Dv, flags, d == "bf16", N + Dk + Dv + rule)
        r, s = ops.scan_fwd(_cuda(q, DT[d]), _cuda(k, DT[d]), _cuda(v, DT[d]), _cuda(a), _cuda(b), _cuda(s0), rule=rule, flags=flags, check=True)
        out[f"R_N{N}_Dk{Dk}_Dv{Dv}"], out[f"S_N{N}_Dk{Dk}_Dv{Dv}"] = r, s
    return out


def _scan_close(R, S, Ro, So, bf16, scale=1.0):
    """tests/test_scan_gpu.py: 1e-4 absolute (relative to the values' scale), plus the bf16 quantisation of a bf16 read-out."""
    assert np.abs(S.cpu().numpy() - So).max() <= 1e-4 * scale
    assert np.all(np.abs(R.float().cpu().numpy() - Ro) <= 1e-4 * scale + (np.abs(Ro) * 2.0 ** -8 if bf16 else 0.0))


def _scan_fwd_check(ops, case, o):
    from oracle import c_oracle
    rule, flags, d = case
    for N, Dk, Dv in SCAN_FWD_SUB:
        q, k, v, a, b, s0 = _scan_inputs(*SCAN_BT, N, 1, Dk, Dv, flags, d == "bf16", N + Dk + Dv + rule)
        Ro, So = c_oracle.scan(q, k, v, a, b, s0, rule, flags, math="f64")
        # (rule delta_parallel is not contractive: 1e-4 of the values' size, as test_segmented_scan_choice_by_shape bounds it)
        scale = max(1.0, float(np.abs(Ro).max()), float(np.abs(So).max())) if rule == 1 else 1.0
        _scan_close(o[f"R_N{N}_Dk{Dk}_Dv{Dv}"], o[f"S_N{N}_Dk{Dk}_Dv{Dv}"], Ro, So, d == "bf16", scale)


SCAN_SHORT, SCAN_LONG = (2, 3, 17, 2, 32), (2, 3, 100, 1, 32)                 # scan_bwd_forms.SHAPE_CASES[1], TOKEN_CASES[0]
NORMALIZER_CASES = [(s, rule, d) for s in (SCAN_SHORT, SCAN_LONG) for rule in (0, 2) for d in ("fp32", "bf16")]


def _normalizer_inputs(case):
    from oracle import gdkvm_oracle as O
    from tests.test_step_normalizer_gpu import _positive_inputs
    (B, T, N, Hh, Dv), rule, d = case
    q, k, v, a, b = _positive_inputs(B, T, N, Hh, 64, Dv, seed=B + T + N + Hh + Dv + rule)
    rng = np.random.default_rng(1)
    s0 = (0.2 * rng.standard_normal((B, Hh, 64, Dv))).astype(np.float32)
    z0 = (0.2 * np.abs(rng.standard_normal((B, Hh, 64)))).astype(np.float32)
    if d == "bf16":
        q, k, v = (O.to_bf16_f32(x) for x in (q, k, v))
    return q, k, v, a, b, s0, z0


def _normalizer_run(ops, case):
    q, k, v, a, b, s0, z0 = _normalizer_inputs(case)
    d = DT[case[2]]
    R, S, Z = ops.scan_fwd_normalizer(_cuda(q, d), _cuda(k, d), _cuda(v, d), _cuda(a), _cuda(b), _cuda(s0), _cuda(z0), rule=case[1], flags=3, eps=1e-6)
    return dict(R=R, S=S, Z=Z)


def _normalizer_check(ops, case, o):
    from oracle import c_oracle
    q, k, v, a, b, s0, z0 = _normalizer_inputs(case)
    Ro, So, Zo = c_oracle.scan_normalizer(q, k, v, a, b, s0, z0, case[1], 3, 1e-6, math="f64")
    assert np.abs(o["S"].cpu().numpy() - So).max() <= 1e-4 and np.abs(o["Z"].cpu().numpy() - Zo).max() <= 1e-4
    scale = max(1.0, float(np.abs(Ro).max()))
    assert np.abs(o["R"].float().cpu().numpy() - Ro).max() <= (1e-4 * scale if case[2] == "fp32" else 3 * 2.0 ** -8 * scale)


# (shape, segments): scan_bwd_forms.GRID_CASES' shape at both segment counts; TOKEN_CASES[1] (130 tokens), and the same with T = 4 for 4 segments
SEGMENTED_CASES = [((2, 4, 49, 1, 80), 2), ((2, 4, 49, 1, 80), 4), ((1, 2, 130, 2, 48), 2), ((1, 4, 130, 2, 48), 4)]


def _segmented_run(ops, case):
    (B, T, N, Hh, Dv), segs = case
    q, k, v, a, b, s0 = _scan_inputs(B, T, N, Hh, 64, Dv, 3, False, B + T + N + Dv)
    R, S = ops.scan_fwd_segmented(*(_cuda(x) for x in (q, k, v, a, b, s0)), segments=segs, flags=3)
    return dict(R=R, S=S)


def _segmented_check(ops, case, o):
    from oracle import c_oracle
    (B, T, N, Hh, Dv), segs = case
    q, k, v, a, b, s0 = _scan_inputs(B, T, N, Hh, 64, Dv, 3, False, B + T + N + Dv)
    Ro, So = c_oracle.scan(q, k, v, a, b, s0, 2, 3, math="f64")                 # test_transition_matrix_and_segmented_scan: 1e-4
    _scan_close(o["R"], o["S"], Ro, So, False)


SCAN_TRAIN_CASES = [s + (2, 3, d, 64) for s in (SCAN_SHORT, SCAN_LONG) for d in ("fp32", "bf16")]      # scan_bwd_forms' case format


def _scan_train_run(ops, case):
    from tests import scan_bwd_forms as Fm
    inp = Fm.make_inputs(case)
    t = Fm.to_device(inp)
    ts = [getattr(t, n).requires_grad_() for n in Fm.NAMES]
    R, S = ops.scan(*ts, inp.rule, inp.flags)
    torch.autograd.backward([R, S], [t.dR, t.dS])
    out = {"d_" + n: x.grad for n, x in zip(Fm.NAMES, ts)}
    out.update(R=R.detach(), S=S.detach())
    return out


def _scan_train_check(ops, case, o):
    from tests import scan_bwd_forms as Fm
    inp = Fm.make_inputs(case)
    if case not in _ref_cache:
        _ref_cache[case] = (Fm.ref_grads(inp), Fm.ref_one_call(inp)[:2])
    ref, (Ro, So) = _ref_cache[case]
    worst = Fm.worst({n: o["d_" + n].float().cpu().numpy() for n in Fm.NAMES}, ref, inp.bf16)
    assert all(v <= 1.0 for v in worst.values()), worst
    _scan_close(o["R"], o["S"], Ro, So, inp.bf16)


STATE_BWD_CASES = [(s, d) for s in [(2, 5, 17, 1, 32), (1, 7, 64, 2, 48)] for d in ("fp32", "bf16")]          # scan_bwd_forms.STATE_BWD_SHAPES


def _state_bwd_parts(case):
    from tests import scan_bwd_forms as Fm
    shape, d = case
    B, T, N, Hh, Dv = shape
    inp = Fm.make_inputs(Fm._c(shape, dtype=d))
    d_hist = np.random.default_rng(sum(shape)).standard_normal((B, T, Hh, 64, Dv)).astype(np.float32)
    return inp, d_hist


def _state_bwd_run(ops, case):
    from tests import scan_bwd_forms as Fm
    B, T, N, Hh, Dv = case[0]
    inp, d_hist = _state_bwd_parts(case)
    t = Fm.to_device(inp)
    ws = ops.new_workspace(B, T, Hh, N, 64, Dv, t.q.device)
    hist = ops.torch.empty((B, T, Hh, 64, Dv), dtype=F32, device=t.q.device)              # (through the module's torch: poisoned when patched)
    R, S = ops.scan_fwd(t.q, t.k, t.v, t.alpha, t.beta, t.s0, workspace=ws, state_hist=hist, flags=3)
    out = ops.scan_state_bwd(t.k, t.v, t.alpha, t.beta, hist, ws, _cuda(d_hist), t.dS, 2, 3)
    res = {"d_" + n: g for n, g in zip(Fm.NAMES[1:], out)}
    res.update(hist=hist, R=R, S=S)
    return res


def _state_bwd_check(ops, case, o):
    from tests import scan_bwd_forms as Fm
    inp, d_hist = _state_bwd_parts(case)
    if case not in _ref_cache:
        _ref_cache[case] = Fm.ref_state_grads(inp, d_hist, True, True)
    ref = _ref_cache[case]
    worst = Fm.worst({n: o["d_" + n].float().cpu().numpy() for n in Fm.NAMES[1:]}, ref, inp.bf16)
    assert all(v <= 1.0 for v in worst.values()), worst


# ---- mask and frame kernels --------------------------------------------------------------------------------------------------------------------
SPLIT_15360 = [(2, 120, 128), (2, 121, 127)]                                    # LAST_LDS, FIRST_WS of the two label kernels' GPU tests
SPLIT_14336 = [(2, 112, 128), (2, 113, 127)]                                    # tests/test_surface_distance_gpu.py
SPLIT_18432 = [(1, 144, 128), (1, 145, 128)]                                    # tests/test_spacing_gpu.py: the mm kernel's own split


def _largest_run(ops, shape):
    from tests.test_largest_component_gpu import _case
    frames, target, _, _ = _case(*shape, 4, 1, 0)
    out, info = ops.largest_component(_cuda(frames), cls=1, connectivity=4, fill=0, target=_cuda(target))
    return dict(out=out, info=info)


def _largest_check(ops, shape, o):
    from tests.test_largest_component_gpu import _case
    _, _, want_out, want_info = _case(*shape, 4, 1, 0)
    assert np.array_equal(o["info"].cpu().numpy(), want_info) and np.array_equal(o["out"].cpu().numpy(), want_out)


def _holes_run(ops, shape):
    from tests.test_fill_holes_gpu import _case
    frames, target, _, _ = _case(*shape, 4, 1, 4)
    out, info = ops.fill_holes(_cuda(frames), cls=1, connectivity=4, max_area=4, target=_cuda(target))
    return dict(out=out, info=info)


def _holes_check(ops, shape, o):
    from tests.test_fill_holes_gpu import _case
    _, _, want_out, want_info = _case(*shape, 4, 1, 4)
    assert np.array_equal(o["info"].cpu().numpy(), want_info) and np.array_equal(o["out"].cpu().numpy(), want_out)


def _surface_run(ops, shape):
    from tests.test_surface_distance_gpu import _case
    mask, target, _ = _case(*shape, 1)
    return dict(surf=ops.surface_distance(_cuda(mask), _cuda(target), cls=1))


def _surface_check(ops, shape, o):
    from tests.test_surface_distance_gpu import _case, _check
    _check(o["surf"], _case(*shape, 1)[2], shape)


def _surface_mm_run(ops, shape):
    from tests.test_spacing_gpu import _case, _sp
    mask, target = _case(*shape)
    return dict(surf=ops.surface_distance_mm(_cuda(mask), _cuda(target), _sp((330, 468)), cls=1))


def _surface_mm_check(ops, shape, o):
    from tests.test_spacing_gpu import _check, _want
    _check(o["surf"], _want(*shape, 330, 468), shape)


def _surface_native_run(ops, case):
    from tests import native_surface_reference as NR
    from tests.test_native_surface_gpu import SPACING, _ragged
    masks, targets, _ = _ragged()
    fm, sizes = NR.pack(masks)
    ft, _ = NR.pack(targets)
    return dict(surf=ops.surface_distance_native(_cuda(fm), _cuda(ft), sizes, masks[0].shape[0], [tuple(s) for s in SPACING], cls=1))


def _surface_native_check(ops, case, o):
    from tests.test_native_surface_gpu import _ragged
    assert np.array_equal(o["surf"].cpu().numpy(), _ragged()[2])


VOTE_SHAPES = [(2, 3, 5, 3, 3, 3), (3, 5, 15, 13, 4, 2)]


def _vote_run(ops, shape):
    from tests.test_temporal_vote_gpu import _case
    mask, target = _case(shape)[:2]
    out, info, counts = ops.temporal_vote(_cuda(mask), shape[4], shape[5], target=_cuda(target))
    return dict(out=out, info=info, counts=counts)


def _vote_check(ops, shape, o):
    from tests.test_temporal_vote_gpu import _case
    _, _, want_out, want_info, want_counts, _ = _case(shape)
    for k, want in (("out", want_out), ("info", want_info), ("counts", want_counts)):
        assert np.array_equal(o[k].cpu().numpy(), want), k


TO_NATIVE_CASES = [(7, 5, 11, 13, 4), (16, 12, 5, 7, 4)]                       # (H, W, h0, w0, ncls): an odd up-scale and a down-scale


def _to_native_inputs(case):
    from tests import native_reference as R
    from tests.test_mask_to_native_gpu import _mask, _target
    H, W, h0, w0, ncls = case
    m = _mask(np.random.default_rng(H * 31 + w0), 2, 3, H, W, ncls)
    sizes = [(h0, w0), (h0, w0)]
    return m, sizes, _target(np.random.default_rng(0), R.offsets(sizes, 3)[1], ncls)


def _to_native_run(ops, case):
    m, sizes, g = _to_native_inputs(case)
    out, counts, _ = ops.mask_to_native(_cuda(m), sizes, case[4], target=_cuda(g))
    return dict(out=out, counts=counts)


def _to_native_check(ops, case, o):
    from tests import native_reference as R
    m, sizes, g = _to_native_inputs(case)
    ref_out, ref_counts = R.mask_to_native(m, sizes, case[4], g)
    assert np.array_equal(o["out"].cpu().numpy(), ref_out) and np.array_equal(o["counts"].cpu().numpy(), ref_counts)


FROM_NATIVE_CASES = [((4, 3), 3, "uint8"), ((8, 8), 1, "float32"), ((4, 3), 3, "bfloat16")]


def _from_native_inputs():
    from tests import native_input_reference as R
    rng = np.random.default_rng(0)                                             # the `ragged` fixture of tests/test_native_input_gpu.py
    clips = [rng.integers(0, 256, (3, h0, w0), dtype=np.uint8) for h0, w0 in ((7, 5), (5, 7), (1, 1), (3, 3), (33, 17), (64, 64), (97, 130))]
    return R.pack(clips)


def _from_native_run(ops, case):
    grid, C, dt = case
    flat, sizes = _from_native_inputs()
    out, _ = ops.frames_from_native(_cuda(flat), sizes, 3, grid=grid, channels=C, dtype=getattr(torch, dt))
    return dict(out=out)


def _from_native_check(ops, case, o):
    from tests import native_input_reference as R
    from tests.test_native_input_gpu import _same
    grid, C, dt = case
    flat, sizes = _from_native_inputs()
    assert _same(o["out"], R.frames_from_native(flat, sizes, 3, grid[0], grid[1], C)[0])


OVERLAY_CASES = [(4, 2, True), (2, 1, False)]                                  # (ncls, width, with a reference mask) on test_overlay_gpu.SMALL


def _overlay_inputs(case):
    from tests.test_overlay_gpu import SMALL, _case
    ncls, w, with_ref = case
    g, m, r = _case(10 * ncls + w, SMALL, 2, ncls)
    return g, m, (r if with_ref else None), SMALL


def _overlay_run(ops, case):
    from tests import overlay_reference as R
    ncls, w, _ = case
    g, m, r, sizes = _overlay_inputs(case)
    got = ops.overlay_native(_cuda(g), _cuda(m), sizes, 2, ncls, reference=None if r is None else _cuda(r), width=w, alpha=96,
                             palette=R.PAL[:ncls].tolist(), reference_palette=R.REF_PAL[:ncls].tolist())
    return dict(out=got)


def _overlay_check(ops, case, o):
    from tests import overlay_reference as R
    ncls, w, _ = case
    g, m, r, sizes = _overlay_inputs(case)
    want = R.overlay_native(g, m, r, sizes, 2, ncls, w, 96, R.PAL[:ncls], R.REF_PAL[:ncls])
    assert o["out"].dtype == torch.uint8 and np.array_equal(o["out"].cpu().numpy().reshape(-1), want.reshape(-1))


# ---- optimiser ---------------------------------------------------------------------------------------------------------------------------------
def _adamw_run(ops, case):
    from tests import test_native_adamw_gpu as A
    state, _ = A._run(A.case(), bucket=False)
    return {f"{k}_{i}": t for k in A.KEYS for i, t in enumerate(state[k])}


def _adamw_check(ops, case, o):
    from tests import test_native_adamw_gpu as A
    c = A.case()
    A._assert_close({k: [o[f"{k}_{i}"] for i in range(len(c.params))] for k in A.KEYS}, c.ref, c.err, what="poisoned")


_T = "tests/test_train_side_gpu.py::"
ENTRIES = [
    Row("bn_act", ("gdkvm_bn_workspace_bytes",), [(s, m) for s in BN_SHAPES for m in ("relu", "res_relu")], _bn_act_run, _bn_act_check,
        _T + "_reference (test_bn_act_forward_backward)"),
    Row("bn_relu_pool", ("gdkvm_bn_workspace_bytes",), BN_SHAPES, _bn_pool_run, _bn_pool_check, _T + "test_batchnorm_relu_maxpool_as_one_op"),
    Row("head", ("gdkvm_head_bwd_workspace_bytes",), [s + (d,) for s in [(2, 32, 9, 5, 4), (1, 64, 7, 7, 8)] for d in (BF16, F32)], _head_run,
        _head_check, _T + "test_head_forward_and_one_pass_backward"),
    Row("wgrad", ("gdkvm_gemm_tn_workspace_bytes",), [(m, d, False) for m in (1001, 2081) for d in (F32, BF16)], _wgrad_run, _wgrad_check,
        _T + "test_hand_written_products_of_the_training_backward"),
    Row("wgrad_colsum", ("gdkvm_gemm_tn_colsum_workspace_bytes",), [(m, d, True) for m in (1001, 2081) for d in (F32, BF16)], _wgrad_run,
        _wgrad_check, _T + "test_token_linear_and_split_k_weight_gradient"),
    Row("conv3x3_wgrad", ("gdkvm_conv3x3_wgrad_workspace_bytes",), [(s, cl) for s in (WG_LARGEST, WG_SMALLEST, WG_TINY) for cl in (False, True)],
        _conv3_run, _conv3_check, "tests/test_wgrad_tiles_gpu.py::ref_wgrad, bound of test_convolution_weight_gradient"),
    Row("conv_wgrad_strided", ("gdkvm_conv_wgrad_strided_workspace_bytes",), [(s, cl) for s in STRIDED_CASES for cl in (False, True)],
        _strided_run, _strided_check, "tests/test_wgrad_tiles_gpu.py::ref_wgrad, bound of test_strided_weight_gradient_any_window"),
    Row("stem_conv", ("gdkvm_stem_wgrad_workspace_bytes",), [(2, 1, 64, 48), (1, 4, 130, 118)], _stem_run, _stem_check,
        _T + "test_training_stem_convolution_on_the_stem_kernel"),
    Row("mask_embed_wgrad", ("gdkvm_mask_embed_wgrad_workspace_bytes",), [(g, d) for g in EMBED_GEOMS for d in (F32, BF16)], _embed_run,
        _embed_check, "tests/test_feedback_train_gpu.py::_wgrad_ref"),
    Row("kpff_fwd", ("gdkvm_kpff_workspace_bytes",), KPFF_CASES, _kpff_fwd_run, _kpff_fwd_check, "tests/test_kpff_argmax_gpu.py (c_oracle.kpff)"),
    Row("kpff", ("gdkvm_kpff_workspace_bytes", "gdkvm_gemm_tn_workspace_bytes", "gdkvm_gemm_tn_colsum_workspace_bytes"), KPFF_CASES,
        _kpff_train_run, _kpff_train_check, "tests/test_kpff_train_forms_gpu.py::test_whole_backward_in_the_large_forms (oracle.torch_ref.kpff)"),
    Row("seg_loss", ("gdkvm_seg_loss_workspace_bytes",), LOSS_CASES, _loss_run(False), _loss_check(False),
        "tests/boundary_reference.py::objective_lowres at weight 0, bounds of test_fused_objective_matches_the_torch_loss"),
    Row("seg_loss_boundary", ("gdkvm_seg_loss_boundary_workspace_bytes", "gdkvm_signed_distance_workspace_bytes"), LOSS_CASES, _loss_run(True),
        _loss_check(True), "tests/boundary_reference.py::objective_lowres (test_fused_boundary_objective)"),
    Row("signed_distance", ("gdkvm_signed_distance_workspace_bytes",), SD_SHAPES, _sd_run, _sd_check, "tests/boundary_reference.py::sd2_reference"),
    Row("scan_fwd", ("gdkvm_scan_workspace_bytes",), SCAN_FWD_CASES, _scan_fwd_run, _scan_fwd_check, "tests/test_scan_gpu.py (c_oracle.scan, TOL)",
        note="each case walks N x Dk x Dv = SCAN_FWD_SUB with check=True"),
    Row("scan_fwd_normalizer", ("gdkvm_scan_normalizer_workspace_bytes",), NORMALIZER_CASES, _normalizer_run, _normalizer_check,
        "tests/test_step_normalizer_gpu.py::test_scan_normalizer_matches_the_oracle_and_carries_z"),
    Row("scan_fwd_segmented", ("gdkvm_scan_segmented_workspace_bytes",), SEGMENTED_CASES, _segmented_run, _segmented_check,
        "tests/test_configs_gpu.py::test_transition_matrix_and_segmented_scan"),
    Row("scan", ("gdkvm_scan_workspace_bytes", "gdkvm_scan_bwd_workspace_bytes", "gdkvm_scan_train_workspace_bytes"), SCAN_TRAIN_CASES,
        _scan_train_run, _scan_train_check, "tests/scan_bwd_forms.py::ref_grads, worst"),
    Row("scan_state_bwd", ("gdkvm_scan_workspace_bytes", "gdkvm_scan_bwd_workspace_bytes"), STATE_BWD_CASES, _state_bwd_run, _state_bwd_check,
        "tests/scan_bwd_forms.py::ref_state_grads, worst"),
    Row("largest_component", ("gdkvm_largest_component_workspace_bytes",), SPLIT_15360, _largest_run, _largest_check,
        "tests/test_largest_component_gpu.py::_case (tests/cc_reference.py)"),
    Row("fill_holes", ("gdkvm_fill_holes_workspace_bytes",), SPLIT_15360, _holes_run, _holes_check,
        "tests/test_fill_holes_gpu.py::_case (tests/holes_reference.py)"),
    Row("surface_distance", ("gdkvm_surface_distance_workspace_bytes",), SPLIT_14336, _surface_run, _surface_check,
        "tests/test_surface_distance_gpu.py::_case, _check"),
    Row("surface_distance_mm", ("gdkvm_surface_distance_mm_workspace_bytes",), SPLIT_14336 + SPLIT_18432, _surface_mm_run, _surface_mm_check,
        "tests/test_spacing_gpu.py::_want, _check"),
    Row("surface_distance_native", ("gdkvm_surface_distance_native_workspace_bytes",), ["ragged"], _surface_native_run, _surface_native_check,
        "tests/test_native_surface_gpu.py::_ragged"),
    Row("temporal_vote", ("gdkvm_temporal_vote_workspace_bytes",), VOTE_SHAPES, _vote_run, _vote_check, "tests/test_temporal_vote_gpu.py::_case"),
    Row("mask_to_native", ("gdkvm_mask_to_native_workspace_bytes",), TO_NATIVE_CASES, _to_native_run, _to_native_check,
        "tests/native_reference.py::mask_to_native"),
    Row("frames_from_native", ("gdkvm_frames_from_native_workspace_bytes",), FROM_NATIVE_CASES, _from_native_run, _from_native_check,
        "tests/native_input_reference.py::frames_from_native, tests/test_native_input_gpu.py::_same"),
    Row("overlay_native", ("gdkvm_overlay_native_workspace_bytes",), OVERLAY_CASES, _overlay_run, _overlay_check,
        "tests/overlay_reference.py::overlay_native"),
    Row("adamw_step", ("gdkvm_adamw_workspace_bytes",), ["parity"], _adamw_run, _adamw_check,
        "tests/test_native_adamw_gpu.py::case, _run, _assert_close"),
]
# row -> the queries that may return no more than the 16-byte floor at some of the row's shapes: the four that are 0 everywhere, the LDS side
# of each LDS / workspace split, and KPFF where the exact arm serves the channel counts.  Every other query of every row must exceed 16.
_LDS_SIDE = {n: ("gdkvm_%s_workspace_bytes" % n,) for n in ("largest_component", "fill_holes", "surface_distance", "surface_distance_mm",
                                                            "signed_distance", "temporal_vote", "mask_to_native", "frames_from_native",
                                                            "overlay_native")}
FLOOR_QUERIES = dict(_LDS_SIDE, kpff_fwd=("gdkvm_kpff_workspace_bytes",), kpff=("gdkvm_kpff_workspace_bytes",),
                     seg_loss_boundary=("gdkvm_signed_distance_workspace_bytes",))
ZERO_SIZE = ("gdkvm_temporal_vote_workspace_bytes", "gdkvm_mask_to_native_workspace_bytes", "gdkvm_frames_from_native_workspace_bytes",
             "gdkvm_overlay_native_workspace_bytes")


def row(name: str) -> Row:
    return next(r for r in ENTRIES if r.name == name)


def covered_queries():
    return {q for r in ENTRIES for q in r.queries}
