"""GPU checks of the native optimiser step (gdkvm_amd/optim.py -> csrc/adamw.hip) against the float64 restatement of its definition
(tests/optim_reference.py): parity over five steps in both access paths, lists longer than one launch, the non-finite guard, determinism,
capture and replay (alone and inside GraphedTrainStep), the state round trip with torch.optim.AdamW, and what step() refuses.

The tolerance of the parity checks is MEASURED, not chosen: the largest element error of torch.optim.AdamW + clip_grad_norm_ in fp32 on the CPU
against the float64 reference on the SAME inputs and options as the comparison it serves (torch_fp32_error: an absolute error does not carry
over to gradients of another scale), times 4 -- the kernel's operation order differs from torch's and its norm is
summed in another order -- plus one fp32 ulp of the value compared.  On the parity inputs torch's fp32 errors are 7.7e-7 (parameters, |p| up to
4.1), 4.7e-9 (exp_avg), 4.5e-11 (exp_avg_sq) and 7.7e-7 (EMA): the bounds are 3.1e-6 / 1.9e-8 / 1.8e-10 / 3.1e-6, each plus the ulp."""
import copy

import pytest
import torch

from tests.optim_reference import adamw_reference, schedule_lr, torch_adamw_run

pytestmark = pytest.mark.gpu

COUNTS = [1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 8193]
SCALES = (0.01, 1.0, 0.01, 1.0, 1.0)
OPTS = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, max_norm=10.0, schedule="cosine", warmup_steps=2, total_steps=5, min_lr_ratio=0.1,
            ema_decay=0.9)
KEYS = ("params", "exp_avg", "exp_avg_sq", "ema")


def torch_fp32_error(params, grads, wds, opts) -> dict:
    """The largest element error of torch.optim.AdamW + clip_grad_norm_ (and a plain fp32 EMA) in fp32 on the CPU against the float64 reference,
    per quantity, on exactly these inputs and options: the yardstick of every comparison with the reference in this file."""
    ref = adamw_reference(params, grads, weight_decays=wds, **opts)
    sched = {k: opts[k] for k in ("schedule", "warmup_steps", "total_steps", "min_lr_ratio", "poly_power") if k in opts}
    lrs = [schedule_lr(t, opts["lr"], **sched) for t in range(1, len(grads) + 1)]
    ps, opt, ema = torch_adamw_run(params, grads, dtype=torch.float32, lr=opts["lr"], betas=opts["betas"], eps=opts["eps"], weight_decays=wds,
                                   max_norm=opts.get("max_norm", 0.0), lrs=lrs, ema_decay=opts.get("ema_decay", 0.0))
    got = {"params": ps, "exp_avg": [opt.state[q]["exp_avg"] for q in ps], "exp_avg_sq": [opt.state[q]["exp_avg_sq"] for q in ps], "ema": ema}
    return {k: max(float((a.detach().double() - b).abs().max()) for a, b in zip(got[k], ref[k])) for k in KEYS if got[k] is not None}


class _Case:
    """The parity inputs (CPU, seeded), their float64 reference and torch's fp32 error against it: computed once, never changed."""

    def __init__(self):
        gen = torch.Generator().manual_seed(1234)
        shapes = [(n,) for n in COUNTS] + [(8, 4, 3, 3)]
        cl = lambda t: t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t
        self.params = [cl(torch.randn(s, generator=gen)) for s in shapes]
        self.grads = [[cl(sc * torch.randn(s, generator=gen)) for s in shapes] for sc in SCALES]
        self.wds = [0.0 if i % 2 == 0 else 0.05 for i in range(len(shapes))]              # half of the tensors get decay 0
        self.ref = adamw_reference(self.params, self.grads, weight_decays=self.wds, **OPTS)
        self.err = torch_fp32_error(self.params, self.grads, self.wds, OPTS)


_CASE = []


def case() -> _Case:
    if not _CASE:
        _CASE.append(_Case())
    return _CASE[0]


def _ulp(ref64: torch.Tensor) -> torch.Tensor:
    a = ref64.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def _assert_close(got: dict, ref: dict, err: dict, keys=KEYS, what=""):
    """|got - ref| <= 4 x torch's fp32 error on these inputs + one fp32 ulp of the value, element by element; prints the figures first."""
    for k in keys:
        worst = 0.0
        for i, (a, r) in enumerate(zip(got[k], ref[k])):
            d = (a.detach().double().cpu() - r).abs()
            worst = max(worst, float(d.max()))
            bound = 4.0 * err[k] + _ulp(r)
            assert bool((d <= bound).all()), (what, k, i, float(d.max()), 4.0 * err[k])
        print(f"{what} {k}: largest error {worst:.3e}, torch fp32 error {err[k]:.3e}, bound 4x = {4.0 * err[k]:.3e} + ulp")


def _device_params(params):
    return [torch.nn.Parameter(p.detach().clone(memory_format=torch.preserve_format).cuda()) for p in params]


def _make(params, wds, **opts):
    from gdkvm_amd.optim import NativeAdamW
    ps = _device_params(params)
    opt = NativeAdamW([{"params": [(f"t{i}", q)], "weight_decay": wd} for i, (q, wd) in enumerate(zip(ps, wds))], **opts)
    return ps, opt


def _state(ps, opt, ema=True) -> dict:
    out = {"params": [q.detach().clone() for q in ps], "exp_avg": [opt.state[q]["exp_avg"].clone() for q in ps],
           "exp_avg_sq": [opt.state[q]["exp_avg_sq"].clone() for q in ps]}
    if ema:
        out["ema"] = [opt.state[q]["ema"].clone() for q in ps]
    return out


def _bits_equal(a: dict, b: dict) -> bool:
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for k in a for x, y in zip(a[k], b[k]))


def _bucket_views(ps):
    """One flat bucket; the view of tensor i starts at an ODD element offset (4 bytes past nothing useful), with the parameter's strides."""
    bucket = torch.zeros(sum(q.numel() + 2 for q in ps) + 1, device="cuda")
    views, off = [], 1
    for q in ps:
        views.append(bucket[off:off + q.numel()].as_strided(q.shape, q.stride()))
        off += q.numel()
        off += 1 if off % 2 == 0 else 2
    assert all(v.data_ptr() % 8 == 4 for v in views)
    return bucket, views


def _run(c: _Case, bucket: bool):
    """The five parity steps; gradients as separate tensors, or as views of one bucket at odd offsets.  Returns (state, per-step stats)."""
    ps, opt = _make(c.params, c.wds, **OPTS)
    views = _bucket_views(ps)[1] if bucket else None
    stats = []
    for grads in c.grads:
        for i, (q, g) in enumerate(zip(ps, grads)):
            if bucket:
                views[i].copy_(g.cuda())
                q.grad = views[i]
            else:
                q.grad = g.cuda()
        kept = [q.grad.clone() for q in ps]
        opt.step()
        assert all(torch.equal(q.grad, k) for q, k in zip(ps, kept))                     # the gradient is read scaled, never written
        stats.append(opt.stats())
    return _state(ps, opt), stats


_RUNS = {}


def runs(key):
    if key not in _RUNS:
        _RUNS[key] = _run(case(), bucket=key == "bucket")
    return _RUNS[key]


def test_parity_over_five_steps_in_both_access_paths(hip):
    c = case()
    coefs = [s[1] for s in c.ref["steps"]]
    assert any(x == 1.0 for x in coefs) and any(x < 0.5 for x in coefs), coefs           # from the reference alone: both regimes are met
    sep, st_sep = runs("separate")
    buc, st_buc = runs("bucket")
    assert _bits_equal(sep, buc) and st_sep == st_buc                                    # 16-byte path and element path: equal bit for bit
    _assert_close(sep, c.ref, c.err, what="separate")
    _assert_close(buc, c.ref, c.err, what="bucket")
    for t, (st, (norm, coef, lr, applied)) in enumerate(zip(st_sep, c.ref["steps"]), 1):
        assert applied and st["step"] == t and st["skipped"] == 0
        lr32 = torch.tensor(lr, dtype=torch.float32)
        ulp = float(torch.nextafter(lr32, torch.tensor(float("inf"))) - lr32)
        print(f"step {t}: lr {st['lr']!r} (reference {lr!r}), norm {st['grad_norm']!r} ({norm!r}), coef {st['clip_coef']!r} ({coef!r})")
        assert abs(st["lr"] - lr) <= ulp
        assert abs(st["grad_norm"] - norm) <= 1e-5 * norm
        assert abs(st["clip_coef"] - coef) <= 1e-5 * coef


def test_more_tensors_than_one_launch_holds(hip):
    """200 tensors of 7 elements: three launches of each table kernel.  The same 1400 values in the same chunk layout -- 200 chunks, the values
    in the first 7 elements of each, zeros behind them (a square of zero adds nothing to a partial) -- held by three tensors, a list that
    fits one launch, give the same partials and so the same norm bit for bit."""
    c = case()
    gen = torch.Generator().manual_seed(77)
    params = [torch.randn(7, generator=gen) for _ in range(200)]
    grads = [[torch.randn(7, generator=gen) for _ in range(200)] for _ in range(2)]
    wds = [0.01 * (i % 3) for i in range(200)]
    opts = dict(OPTS, max_norm=20.0)
    ref = adamw_reference(params, grads, weight_decays=wds, **opts)
    assert ref["steps"][0][1] < 1.0                                                      # the clip is active: the norm reaches the update
    ps, opt = _make(params, wds, **opts)
    norms = []
    for gs in grads:
        for q, g in zip(ps, gs):
            q.grad = g.cuda()
        opt.step()
        norms.append(opt.stats()["grad_norm"])
    _assert_close(_state(ps, opt), ref, torch_fp32_error(params, grads, wds, opts), what="200 tensors")
    assert opt.stats()["step"] == 2
    chunk = 4096
    big = [torch.zeros(n * chunk) for n in (67, 67, 66)]
    flat = torch.stack(grads[0])                                                         # [200, 7]
    for b, lo in zip(big, (0, 67, 134)):
        b.view(-1, chunk)[:, :7] = flat[lo:lo + b.numel() // chunk]
    qs, opt3 = _make([torch.zeros_like(b) for b in big], [0.0] * 3, **opts)
    for q, b in zip(qs, big):
        q.grad = b.cuda()
    opt3.step()
    assert opt3.stats()["grad_norm"] == norms[0]                                         # bit-equal: float == float


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_gradient_skips_the_step(hip, bad):
    c = case()
    ps, opt = _make(c.params, c.wds, **OPTS)

    def step(grads, poison=None):
        for i, (q, g) in enumerate(zip(ps, grads)):
            g = g.clone()
            if poison is not None and i == 7:
                g[4000] = poison                                                         # a value, in the last quad's neighbourhood of a 4095-element tensor
            q.grad = g.cuda()
        opt.step()

    step(c.grads[1])
    before, st0 = _state(ps, opt), opt.stats()
    step(c.grads[2], poison=bad)
    after, st1 = _state(ps, opt), opt.stats()
    assert _bits_equal(before, after)                                                    # parameters, moments and EMA: untouched
    assert st1["skipped"] == 1 and st1["step"] == st0["step"] == 1 and st1["clip_coef"] == 0.0
    assert not torch.isfinite(torch.tensor(st1["grad_norm"]))
    step(c.grads[3])
    seen = [c.grads[1], c.grads[3]]                                                      # the reference never saw the bad step
    ref = adamw_reference(c.params, seen, weight_decays=c.wds, **OPTS)
    _assert_close(_state(ps, opt), ref, torch_fp32_error(c.params, seen, c.wds, OPTS), what=f"after a skipped step ({bad})")
    st2 = opt.stats()
    assert st2["step"] == 2 and st2["skipped"] == 1 and abs(st2["lr"] - ref["steps"][1][2]) <= 1e-9


def test_the_same_steps_twice_give_equal_bits(hip):
    first, st_first = runs("separate")
    again, st_again = _run(case(), bucket=False)
    assert _bits_equal(first, again) and st_first == st_again


def test_captured_step_replays_like_eager_steps(hip):
    """One eager step creates the state (as with any capturable optimiser), then step() is captured on static gradient buffers and replayed 4
    times with the buffers refilled: equal, bit for bit, to 4 more eager steps, and the learning rate follows the schedule from replay to replay."""
    c = case()
    opts = dict(OPTS, total_steps=6)
    sched = {k: opts[k] for k in ("schedule", "warmup_steps", "total_steps", "min_lr_ratio")}
    eager_ps, eager = _make(c.params, c.wds, **opts)
    graph_ps, graphed = _make(c.params, c.wds, **opts)
    static = [g.cuda() for g in c.grads[0]]
    for q, e, s in zip(graph_ps, eager_ps, static):
        q.grad = s
        e.grad = s.clone()
    eager.step()
    graphed.step()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.step()
    assert graphed.stats()["step"] == 1                                                  # the capture itself ran nothing
    lrs = []
    for k in range(1, 5):
        for s, e, new in zip(static, eager_ps, c.grads[k]):
            s.copy_(new.cuda())
            e.grad = new.cuda()
        g.replay()
        eager.step()
        assert graphed.stats() == eager.stats()
        lrs.append(graphed.stats()["lr"])
    assert _bits_equal(_state(graph_ps, graphed), _state(eager_ps, eager))
    want = [schedule_lr(t, opts["lr"], **sched) for t in range(2, 6)]
    assert lrs == pytest.approx(want, rel=1e-12) and len(set(lrs)) == 4                  # warm-up end, then down the cosine
    fresh_ps, fresh = _make(c.params, c.wds, **opts)
    for q, s in zip(fresh_ps, static):
        q.grad = s
    with pytest.raises(RuntimeError, match="eager step first"):                          # state is never created inside a capture
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            fresh.step()


def test_graphed_train_step_with_the_native_optimiser(hip, monkeypatch):
    """The whole training step with NativeAdamW (clipping, warm-up, cosine): GraphedTrainStep with 2 warm-up steps and 3 replays against 5 eager
    train_steps from the same seed -- losses and every parameter equal bit for bit, and both counters at 5.
    At these widths most convolutions run in the framework's library (the hand-written training kernels serve the default widths), and its
    default backward solvers do not repeat their own bits: two EAGER runs with torch.optim.AdamW end in different parameters (measured: losses
    0.98089 / 0.98095 after five steps).  The library's deterministic solvers are asked for, so that the comparison speaks about the step."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    from gdkvm_amd.optim import NativeAdamW
    from gdkvm_amd.train import GraphedTrainStep, train_step
    torch.manual_seed(11)
    a = GDKVM(GDKVMConfig(widths=(16, 32, 64), pixel_dim=64, value_dim=64)).train().cuda().to(memory_format=torch.channels_last)
    b = copy.deepcopy(a)
    gen = torch.Generator().manual_seed(5)
    frames = [torch.rand(2, 3, 3, 64, 64, generator=gen).cuda() for _ in range(4)]
    yy, xx = torch.meshgrid(torch.arange(64), torch.arange(64), indexing="ij")
    target = ((((yy - 32) / 19.0) ** 2 + ((xx - 32) / 13.0) ** 2) < 1).long().expand(2, 3, 64, 64).contiguous().cuda()
    kw = dict(lr=1e-3, max_norm=0.5, schedule="cosine", warmup_steps=3, total_steps=5, min_lr_ratio=0.1)
    opt_a, opt_b = NativeAdamW(list(a.named_parameters()), **kw), NativeAdamW(list(b.named_parameters()), **kw)
    order = [0, 0, 1, 2, 3]                                                              # (the warm-up steps run on the batch given at construction)
    eager = [float(train_step(a, opt_a, frames[i], target, torch.bfloat16)) for i in order]
    gstep = GraphedTrainStep(b, opt_b, frames[0], target, torch.bfloat16, warmup=2)
    graphed = [float(gstep(frames[i], target)) for i in order[2:]]
    torch.cuda.synchronize()
    assert graphed == eager[2:], (graphed, eager)
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32)), n
    sa, sb = opt_a.stats(), opt_b.stats()
    assert sa["step"] == 5 and sb["step"] == 5 and sa == sb and sa["skipped"] == 0
    print("GraphedTrainStep + NativeAdamW:", eager, sa)


def test_state_round_trip_with_itself_and_with_torch(hip):
    c = case()
    ps, opt = _make(c.params, c.wds, **OPTS)
    for grads in c.grads[:2]:
        for q, g in zip(ps, grads):
            q.grad = g.cuda()
        opt.step()
    sd = copy.deepcopy(opt.state_dict())
    assert all(float(st["step"]) == 2.0 and set(st) == {"step", "exp_avg", "exp_avg_sq", "ema"} for st in sd["state"].values())
    ps2, opt2 = _make([q.detach().cpu() for q in ps], c.wds, **OPTS)
    opt2.load_state_dict(sd)
    assert opt2.stats()["step"] == 2
    for q, q2, g in zip(ps, ps2, c.grads[2]):
        q.grad = g.cuda()
        q2.grad = g.cuda()
    opt.step()
    opt2.step()
    assert _bits_equal(_state(ps, opt), _state(ps2, opt2)) and opt.stats() == opt2.stats() and opt2.stats()["step"] == 3

    # into torch.optim.AdamW(fused=True): clipping off, constant schedule, no EMA -- the third step within the parity tolerance
    plain = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8)
    ps, opt = _make(c.params, c.wds, **plain)
    for grads in c.grads[:2]:
        for q, g in zip(ps, grads):
            q.grad = g.cuda()
        opt.step()
    tps = _device_params([q.detach().cpu() for q in ps])
    topt = torch.optim.AdamW([{"params": [q], "weight_decay": wd} for q, wd in zip(tps, c.wds)], fused=True, **plain)
    topt.load_state_dict(opt.state_dict())
    for q, g in zip(tps, c.grads[2]):
        q.grad = g.cuda()
    topt.step()
    ref = adamw_reference(c.params, c.grads[:3], weight_decays=c.wds, **plain)
    got = {"params": tps, "exp_avg": [topt.state[q]["exp_avg"] for q in tps], "exp_avg_sq": [topt.state[q]["exp_avg_sq"] for q in tps]}
    _assert_close(got, ref, torch_fp32_error(c.params, c.grads[:3], c.wds, plain), keys=("params", "exp_avg", "exp_avg_sq"),
                  what="native state in torch.optim.AdamW")
    assert all(float(topt.state[q]["step"]) == 3.0 for q in tps)
    # ... and the other way round: torch's state after those three steps resumes here
    ps3, opt3 = _make([q.detach().cpu() for q in tps], c.wds, **plain)
    opt3.load_state_dict(topt.state_dict())
    assert opt3.stats()["step"] == 3
    for q, g in zip(ps3, c.grads[3]):
        q.grad = g.cuda()
    opt3.step()
    ref4 = adamw_reference(c.params, c.grads[:4], weight_decays=c.wds, **plain)
    _assert_close(_state(ps3, opt3, ema=False), ref4, torch_fp32_error(c.params, c.grads[:4], c.wds, plain), keys=("params", "exp_avg", "exp_avg_sq"),
                  what="torch state in NativeAdamW")


def test_step_refuses_what_it_cannot_pair_by_address(hip):
    from gdkvm_amd.optim import NativeAdamW
    good = torch.nn.Parameter(torch.zeros(8, device="cuda"))
    good.grad = torch.zeros(8, device="cuda")
    half = torch.nn.Parameter(torch.zeros(8, device="cuda", dtype=torch.bfloat16))
    half.grad = torch.zeros_like(half)
    with pytest.raises(RuntimeError, match="'half'.*bfloat16"):
        NativeAdamW([("good", good), ("half", half)]).step()
    weight = torch.nn.Parameter(torch.zeros(8, 4, 3, 3, device="cuda").contiguous(memory_format=torch.channels_last))
    weight.grad = torch.zeros(8, 4, 3, 3, device="cuda")                                  # contiguous: other strides than the parameter's
    with pytest.raises(RuntimeError, match="'weight'.*gradient.*strides"):
        NativeAdamW([("good", good), ("weight", weight)]).step()
    host = torch.nn.Parameter(torch.zeros(8))
    host.grad = torch.zeros(8)
    with pytest.raises(RuntimeError, match="'host'.*GPU"):
        NativeAdamW([("good", good), ("host", host)]).step()
    with pytest.raises(ValueError, match="group 1.*betas"):
        NativeAdamW([{"params": [good]}, {"params": [weight], "betas": (0.5, 0.9)}])
    sparse = torch.nn.Parameter(torch.zeros(16, device="cuda")[::2])                      # not dense
    sparse.grad = torch.zeros(16, device="cuda")[::2]
    with pytest.raises(RuntimeError, match="'gappy'.*not dense"):
        NativeAdamW([("good", good), ("gappy", sparse)]).step()
    opt = NativeAdamW([("good", good), ("idle", torch.nn.Parameter(torch.zeros(3, device="cuda")))])
    opt.step()                                                                            # a parameter without a gradient is skipped
    assert opt.stats()["step"] == 1 and len(opt.state) == 1
