"""CPU checks of the native optimiser step (gdkvm_amd/optim.py, csrc/adamw.hip): the float64 reference of tests/optim_reference.py against
torch.optim.AdamW and clip_grad_norm_, the schedules at their corners, the `optim:` section of the configuration, the state layout shared with
torch.optim.AdamW, and the argument checks of the C entry (which come before any device call)."""
import ctypes
import math
import os

import pytest
import torch

from tests.optim_reference import adamw_reference, clip_coef, schedule_lr, torch_adamw_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1,), (3,), (5, 7), (4, 3, 3, 3), (257,)]


def _inputs(steps=4, scales=None, seed=0):
    gen = torch.Generator().manual_seed(seed)
    params = [torch.randn(s, generator=gen) for s in SHAPES]
    scales = scales or [1.0] * steps
    grads = [[sc * torch.randn(s, generator=gen) for s in SHAPES] for sc in scales]
    wds = [0.01 if i % 2 else 0.0 for i in range(len(SHAPES))]
    return params, grads, wds


def _close64(a, b):
    return all(torch.allclose(x.double(), y.double(), rtol=1e-12, atol=1e-14) for x, y in zip(a, b))


def test_reference_is_torch_adamw_in_float64():
    params, grads, wds = _inputs()
    ref = adamw_reference(params, grads, lr=1e-2, weight_decays=wds)
    ps, opt, _ = torch_adamw_run(params, grads, dtype=torch.float64, lr=1e-2, weight_decays=wds)
    assert _close64(ref["params"], ps)
    assert _close64(ref["exp_avg"], [opt.state[q]["exp_avg"] for q in ps])
    assert _close64(ref["exp_avg_sq"], [opt.state[q]["exp_avg_sq"] for q in ps])
    assert ref["step"] == 4 and all(s[1] == 1.0 and s[3] for s in ref["steps"])


def test_reference_clipping_is_clip_grad_norm():
    params, grads, wds = _inputs(scales=[0.01, 1.0, 0.01, 1.0])
    ref = adamw_reference(params, grads, lr=1e-2, weight_decays=wds, max_norm=1.0)
    coefs = [s[1] for s in ref["steps"]]
    assert coefs[0] == 1.0 and coefs[2] == 1.0 and coefs[1] < 0.5 and coefs[3] < 0.5      # both regimes are met
    ps, opt, _ = torch_adamw_run(params, grads, dtype=torch.float64, lr=1e-2, weight_decays=wds, max_norm=1.0)
    assert _close64(ref["params"], ps)
    assert _close64(ref["exp_avg_sq"], [opt.state[q]["exp_avg_sq"] for q in ps])


def test_reference_skips_a_non_finite_step_and_keeps_an_ema():
    params, grads, wds = _inputs(steps=3)
    bad = [g.clone() for g in grads[1]]
    bad[2][1, 1] = float("inf")
    with_bad = adamw_reference(params, [grads[0], bad, grads[2]], lr=1e-2, weight_decays=wds, ema_decay=0.9)
    without = adamw_reference(params, [grads[0], grads[2]], lr=1e-2, weight_decays=wds, ema_decay=0.9)
    assert with_bad["step"] == 2 and with_bad["skipped"] == 1 and not with_bad["steps"][1][3]
    assert all(torch.equal(a, b) for k in ("params", "exp_avg", "exp_avg_sq", "ema") for a, b in zip(with_bad[k], without[k]))
    one = adamw_reference(params, grads[:1], lr=1e-2, weight_decays=wds, ema_decay=0.9)
    assert _close64(one["ema"], [0.9 * p.double() + 0.1 * q for p, q in zip(params, one["params"])])


@pytest.mark.parametrize("schedule", ["constant", "cosine", "poly"])
def test_schedules_at_their_corners(schedule):
    lr, W, N, r, power = 2e-3, 4, 20, 0.1, 0.9
    f = lambda t: schedule_lr(t, lr, schedule, W, N, r, power)
    assert f(1) == lr / W and f(W) == lr                                     # t = 1, W: the linear warm-up reaches lr exactly
    s = 1.0 / (N - W)
    at_w1 = {"constant": lr, "cosine": lr * (r + (1 - r) * 0.5 * (1 + math.cos(math.pi * s))), "poly": lr * (r + (1 - r) * (1 - s) ** power)}
    assert f(W + 1) == pytest.approx(at_w1[schedule], rel=1e-15)             # t = W + 1: one step into the decay
    end = lr if schedule == "constant" else lr * r
    assert f(N) == pytest.approx(end, rel=1e-12) and f(N + 1) == pytest.approx(end, rel=1e-12)      # t = N, N + 1: the floor, and it stays
    first = lr if schedule == "constant" else f_no_warmup(lr, schedule, N, r, power)
    assert schedule_lr(1, lr, schedule, 0, N, r, power) == pytest.approx(first, rel=1e-15)          # W = 0: no warm-up, the decay starts at once
    assert schedule_lr(3, lr, schedule, 0, 0, r, power) == pytest.approx(end, rel=1e-12)            # N = 0: past the end from the first step
    assert clip_coef(10.0, 0.0) == 1.0 and clip_coef(0.5, 1.0) == 1.0 and clip_coef(4.0, 1.0) == 1.0 / (4.0 + 1e-6)


def f_no_warmup(lr, schedule, N, r, power):
    s = 1.0 / N
    return lr * (r + (1 - r) * (0.5 * (1 + math.cos(math.pi * s)) if schedule == "cosine" else (1 - s) ** power))


# ---- configuration -------------------------------------------------------------------------------------------------------------------------
def test_optim_config_defaults_and_shipped_yaml():
    from gdkvm_amd.config import OptimCfg, load_config
    want = dict(kind="torch", weight_decay=0.01, betas=[0.9, 0.999], eps=1e-8, decay_1d=True, clip_norm=0.0, schedule="constant", warmup_steps=0,
                min_lr_ratio=0.0, poly_power=0.9, ema_decay=0.0)
    assert load_config().to_dict()["optim"] == want
    assert load_config(os.path.join(ROOT, "config", "config_gdkvm_01.yaml")).to_dict()["optim"] == want
    assert OptimCfg().weight_decay == torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))]).defaults["weight_decay"]
    cfg = load_config(None, ["optim.kind=native", "optim.clip_norm=1", "optim.schedule=cosine", "optim.warmup_steps=100", "optim.decay_1d=false",
                             "optim.ema_decay=0.999", "optim.min_lr_ratio=0.01", "optim.betas=[0.8,0.99]"])
    assert cfg.optim.kind == "native" and cfg.optim.clip_norm == 1.0 and isinstance(cfg.optim.clip_norm, float) and cfg.optim.decay_1d is False
    assert cfg.optim.betas == [0.8, 0.99] and cfg.optim.ema_decay == 0.999 and cfg.optim.warmup_steps == 100
    # the commented-out block of the shipped file is a valid section once uncommented
    import yaml
    lines = open(os.path.join(ROOT, "config", "config_gdkvm_01.yaml")).read().splitlines()
    i0 = next(i for i, ln in enumerate(lines) if ln.startswith("# optim:"))
    block = [lines[i0][2:]]
    for ln in lines[i0 + 1:]:
        if not ln.startswith("#   "):
            break
        block.append(ln[2:])
    section = yaml.safe_load("\n".join(block))["optim"]
    assert set(section) == set(want) and section["kind"] == "native"
    ov = [f"optim.{k}={v if not isinstance(v, bool) else str(v).lower()}" for k, v in section.items()]
    assert load_config(None, ov).optim.schedule == "cosine"


@pytest.mark.parametrize("override", [
    "optim.kind=sgd", "optim.weight_decay=-0.1", "optim.weight_decay=.nan", "optim.eps=-1", "optim.eps=.inf", "optim.betas=[0.9]", "optim.betas=[0.9,1.0]",
    "optim.betas=[-0.1,0.9]", "optim.betas=0.9", "optim.decay_1d=1", "optim.clip_norm=-1", "optim.clip_norm=true", "optim.schedule=linear",
    "optim.warmup_steps=-1", "optim.warmup_steps=1.5", "optim.min_lr_ratio=1.5", "optim.min_lr_ratio=-0.1", "optim.poly_power=-1",
    "optim.ema_decay=1.0", "optim.ema_decay=-0.5"])
def test_bad_optim_values_are_refused(override):
    from gdkvm_amd.config import load_config
    with pytest.raises(ValueError, match=r"optim\."):
        load_config(None, ["optim.kind=native", override])


@pytest.mark.parametrize("override", ["optim.decay_1d=false", "optim.clip_norm=1.0", "optim.schedule=cosine", "optim.warmup_steps=10",
                                      "optim.min_lr_ratio=0.1", "optim.poly_power=2.0", "optim.ema_decay=0.99"])
def test_native_only_keys_are_refused_under_kind_torch(override):
    from gdkvm_amd.config import load_config
    with pytest.raises(ValueError, match="kind = native"):
        load_config(None, [override])
    assert load_config(None, ["optim.kind=native", override]).optim.kind == "native"
    assert load_config(None, ["optim.weight_decay=0.05", "optim.betas=[0.8,0.9]", "optim.eps=1e-6"]).optim.weight_decay == 0.05     # both kinds


# ---- the optimiser class on the host --------------------------------------------------------------------------------------------------------
def test_state_layout_is_torch_adamws():
    """A torch.optim.AdamW state dict loads into NativeAdamW (same state names, the step counter taken from it), NativeAdamW's loads back into
    torch.optim.AdamW, and the step torch takes from there is the reference's third step."""
    from gdkvm_amd.optim import NativeAdamW
    params, grads, wds = _inputs(steps=3)
    ps, topt, _ = torch_adamw_run(params, grads[:2], dtype=torch.float32, lr=1e-2, weight_decays=[0.01] * len(params))
    ref2 = adamw_reference(params, grads[:2], lr=1e-2)
    qs = [torch.nn.Parameter(q.detach().clone()) for q in ps]
    nopt = NativeAdamW([{"params": [q]} for q in qs], lr=1e-2)
    nopt.load_state_dict(topt.state_dict())
    assert nopt.stats()["step"] == 2
    for q, r_m, r_v in zip(qs, ref2["exp_avg"], ref2["exp_avg_sq"]):
        st = nopt.state[q]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and st["exp_avg"].stride() == q.stride()
        assert torch.allclose(st["exp_avg"].double(), r_m, rtol=1e-5, atol=1e-8) and torch.allclose(st["exp_avg_sq"].double(), r_v, rtol=1e-5, atol=1e-10)
    assert all(g["max_norm"] == 0.0 and g["schedule"] == "constant" for g in nopt.param_groups)       # torch's groups carry none of these
    sd = nopt.state_dict()
    assert all(float(st["step"]) == 2.0 for st in sd["state"].values())
    back = torch.optim.AdamW([{"params": [torch.nn.Parameter(q.detach().clone())]} for q in qs], lr=1e-2)
    back.load_state_dict(sd)
    bps = [g["params"][0] for g in back.param_groups]
    for q, g in zip(bps, grads[2]):
        q.grad = g.clone()
    back.step()
    ref3 = adamw_reference(params, grads, lr=1e-2)
    assert all(torch.allclose(q.double(), r, rtol=1e-5, atol=1e-6) for q, r in zip(bps, ref3["params"]))


def test_groups_may_differ_in_weight_decay_only_and_cpu_tensors_are_refused():
    from gdkvm_amd.optim import NativeAdamW
    a, b = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))
    NativeAdamW([{"params": [a], "weight_decay": 0.0}, {"params": [b]}], lr=1e-3)
    for key, val in (("betas", (0.8, 0.999)), ("lr", 1e-2), ("eps", 1e-6), ("max_norm", 1.0), ("schedule", "cosine"), ("ema_decay", 0.5)):
        with pytest.raises(ValueError, match=key):
            NativeAdamW([{"params": [a]}, {"params": [b], key: val}], lr=1e-3)
    with pytest.raises(ValueError, match="betas"):
        NativeAdamW([a], betas=(0.9, 1.0))
    with pytest.raises(ValueError, match="schedule"):
        NativeAdamW([a], schedule="linear")
    opt = NativeAdamW([("first", a), ("second", b)], lr=1e-3)
    b.grad = torch.zeros(2, 2)
    with pytest.raises(RuntimeError, match="'second'.*GPU"):                 # a CPU parameter: named, and no CPU path
        opt.step()
    assert opt.stats()["step"] == 0 and not opt.state


# ---- the C entry's argument checks (before any device call: they run on a machine without a GPU) -----------------------------------------------
def _c_call(lib, **over):
    n = over.pop("n", 2)
    a = {"params": [0x10000, 0x20000], "grads": [0x30000, 0x40004], "exp_avg": [0x50000, 0x60000], "exp_avg_sq": [0x70000, 0x80000],
         "ema": [0x90000, 0], "counts": [5, 4097], "decays": [0.01, 0.0], "state": 0xA0000, "workspace": 0xB0000, "workspace_bytes": None,
         "lr": 1e-3, "beta1": 0.9, "beta2": 0.999, "eps": 1e-8, "max_norm": 1.0, "ema_decay": 0.9, "min_lr_ratio": 0.1, "poly_power": 0.9,
         "warmup_steps": 2, "total_steps": 10, "schedule": 1}
    a.update(over)
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = lib.gdkvm_adamw_workspace_bytes(n, sum(max(c, 0) for c in (a["counts"] or [4096 * 4])[:max(n, 0)]))
    u64 = lambda v: None if v is None else (ctypes.c_uint64 * len(v))(*v)
    keep = [u64(a[k]) for k in ("params", "grads", "exp_avg", "exp_avg_sq", "ema")]
    counts = None if a["counts"] is None else (ctypes.c_int64 * len(a["counts"]))(*a["counts"])
    decays = None if a["decays"] is None else (ctypes.c_float * len(a["decays"]))(*a["decays"])
    ptr = lambda x: None if x is None else ctypes.cast(x, ctypes.c_void_p)
    return lib.gdkvm_adamw_step(*[ptr(k) for k in keep], ptr(counts), ptr(decays), n, a["state"], a["workspace"], a["workspace_bytes"],
                                a["lr"], a["beta1"], a["beta2"], a["eps"], a["max_norm"], a["ema_decay"], a["min_lr_ratio"], a["poly_power"],
                                a["warmup_steps"], a["total_steps"], a["schedule"], None)


_BAD = {
    "null parameter": dict(params=[0x10000, 0]), "null gradient": dict(grads=[0, 0x40004]), "null exp_avg": dict(exp_avg=[0x50000, 0]),
    "null exp_avg_sq": dict(exp_avg_sq=[0, 0x80000]), "null host array": dict(grads=None), "null counts": dict(counts=None),
    "misaligned parameter": dict(params=[0x10002, 0x20000]), "misaligned gradient": dict(grads=[0x30000, 0x40001]),
    "misaligned exp_avg": dict(exp_avg=[0x50003, 0x60000]), "misaligned exp_avg_sq": dict(exp_avg_sq=[0x70000, 0x80002]),
    "misaligned ema": dict(ema=[0x90001, 0]), "count 0": dict(counts=[5, 0]), "count < 0": dict(counts=[-5, 4097]),
    "short workspace": dict(workspace_bytes=8), "null workspace": dict(workspace=None), "null state": dict(state=None),
    "beta1 = 1": dict(beta1=1.0), "beta1 < 0": dict(beta1=-0.1), "beta2 = 1": dict(beta2=1.0), "beta2 nan": dict(beta2=float("nan")),
    "lr < 0": dict(lr=-1e-3), "lr nan": dict(lr=float("nan")), "lr inf": dict(lr=float("inf")), "eps < 0": dict(eps=-1e-8), "eps inf": dict(eps=float("inf")),
    "decay < 0": dict(decays=[0.01, -0.1]), "decay nan": dict(decays=[float("nan"), 0.0]), "max_norm < 0": dict(max_norm=-1.0),
    "max_norm nan": dict(max_norm=float("nan")), "ema decay < 0": dict(ema_decay=-0.1), "ema decay inf": dict(ema_decay=float("inf")),
    "unknown schedule": dict(schedule=3), "schedule < 0": dict(schedule=-1), "min_lr_ratio > 1": dict(min_lr_ratio=1.5),
    "min_lr_ratio < 0": dict(min_lr_ratio=-0.1), "tensors < 0": dict(n=-1),
}


@pytest.mark.parametrize("case", sorted(_BAD))
def test_c_entry_refuses_bad_arguments(case):
    from gdkvm_amd import build, ops
    build.build()
    lib = ops.load()
    assert _c_call(lib, **_BAD[case]) == -1, case                            # GDKVM_ERR_SHAPE
    assert b"adamw_step" in lib.gdkvm_last_error()


def test_c_entry_empty_list_and_workspace_size():
    from gdkvm_amd import build, ops
    build.build()
    lib = ops.load()
    assert _c_call(lib, n=0) == 0                                            # GDKVM_OK, no launch (and no device here)
    assert _c_call(lib, n=0, params=None, grads=None, exp_avg=None, exp_avg_sq=None, ema=None, counts=None, decays=None, workspace=None,
                   workspace_bytes=0, state=None) == 0
    # one fp32 partial per 4096-element chunk: the bound is total / 4096 + tensors
    assert lib.gdkvm_adamw_workspace_bytes(2, 5 + 4097) >= 4 * (1 + 2)
    assert lib.gdkvm_adamw_workspace_bytes(74, 3997764) == 4 * (3997764 // 4096 + 74)
    assert lib.gdkvm_adamw_workspace_bytes(0, 0) == 0
