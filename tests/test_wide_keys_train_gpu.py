"""Training at per-head key widths 72 .. 256 (gdkvm_scan_train_fwd / _bwd on the wide-key kernels, csrc/gdr_general.hip and
csrc/gdr_general_bwd.hip): scan gradients against fp64 autograd through oracle/torch_ref.py with the tolerances of test_backward_gpu.py,
bit-identity with the inference forward and across backward calls, module gradients against oracle/model_plain.py, and the graphed
training step at key_dim = 128."""
import numpy as np
import pytest
import torch

from oracle import torch_ref as TR
from tests.util import make_scan_inputs

pytestmark = pytest.mark.gpu


def _ref_grads(q, k, v, a, b, s0, dR, dS, rule, flags):
    ts = [torch.from_numpy(np.asarray(x, np.float64)).requires_grad_() for x in (q, k, v, a, b)]
    st = None if s0 is None else torch.from_numpy(np.asarray(s0, np.float64)).requires_grad_()
    R, S = TR.scan(*ts, st, rule, flags)
    loss = (R * torch.from_numpy(dR).double()).sum()
    if dS is not None:
        loss = loss + (S * torch.from_numpy(dS).double()).sum()
    loss.backward()
    return [t.grad.numpy() for t in ts] + ([] if st is None else [st.grad.numpy()])


def _hip_grads(hip, q, k, v, a, b, s0, dR, dS, rule, flags, dtype=torch.float32):
    dev = lambda x, dt=None: torch.from_numpy(np.ascontiguousarray(x)).cuda().to(dt or torch.float32)
    tq, tk, tv = (dev(x, dtype).requires_grad_() for x in (q, k, v))
    ta, tb = (dev(x).requires_grad_() for x in (a, b))
    ts0 = None if s0 is None else dev(s0).requires_grad_()
    R, S = hip.scan(tq, tk, tv, ta, tb, ts0, rule, flags)
    if dS is None:
        torch.autograd.backward([R], [dev(dR, dtype)])
    else:
        torch.autograd.backward([R, S], [dev(dR, dtype), dev(dS)])
    return [t.grad.float().cpu().numpy() for t in [tq, tk, tv, ta, tb] + ([] if ts0 is None else [ts0])]


def _check(got, ref, names="q k v alpha beta s0"):
    for name, g, r in zip(names.split(), got, ref):
        assert np.abs(g - r).max() <= 1e-4 * max(1.0, np.abs(r).max()), (name, np.abs(g - r).max(), np.abs(r).max())


@pytest.mark.parametrize("Dk", [72, 128, 256])
@pytest.mark.parametrize("rule", [0, 1, 2])
@pytest.mark.parametrize("flags", [0, 3])
def test_wide_key_scan_backward(hip, Dk, rule, flags):
    B, T, N, Hh, Dv = 2, 3, 49, 1, 32
    q, k, v, a, b = make_scan_inputs(B, T, N, Hh, Dk, Dv, seed=Dk + 10 * rule + flags, normalized=not flags, logits=bool(flags), corr=0.5)
    rng = np.random.default_rng(Dk + rule)
    s0 = (0.3 * rng.standard_normal((B, Hh, Dk, Dv))).astype(np.float32)
    dR = rng.standard_normal((B, T, N, Hh, Dv)).astype(np.float32)
    dS = rng.standard_normal((B, Hh, Dk, Dv)).astype(np.float32)
    _check(_hip_grads(hip, q, k, v, a, b, s0, dR, dS, rule, flags), _ref_grads(q, k, v, a, b, s0, dR, dS, rule, flags))


@pytest.mark.parametrize("shape", [(1, 16, 128), (64, 80, 72), (65, 256, 128), (130, 16, 256), (256, 80, 136)])
def test_wide_key_scan_backward_shapes(hip, shape):
    """Frames of 1 .. 256 tokens (over the 64-token chunks the kernels stage norms and gates in), two heads, no input state and no
    gradient on the final state."""
    N, Dv, Dk = shape
    B, T, Hh = 1, 2, 2
    q, k, v, a, b = make_scan_inputs(B, T, N, Hh, Dk, Dv, seed=sum(shape), normalized=False, logits=True, corr=0.7)
    dR = np.random.default_rng(N).standard_normal((B, T, N, Hh, Dv)).astype(np.float32)
    _check(_hip_grads(hip, q, k, v, a, b, None, dR, None, 2, 3), _ref_grads(q, k, v, a, b, None, dR, None, 2, 3), "q k v alpha beta")


def test_wide_key_scan_backward_bf16_io(hip):
    """bf16 tensors: the gradient of the exact-fp32 function of the bf16-rounded inputs, returned in bf16."""
    from oracle import gdkvm_oracle as O
    B, T, N, Hh, Dk, Dv = 2, 3, 49, 1, 128, 64
    q, k, v, a, b = make_scan_inputs(B, T, N, Hh, Dk, Dv, seed=44, normalized=False, logits=True)
    rng = np.random.default_rng(45)
    s0 = (0.3 * rng.standard_normal((B, Hh, Dk, Dv))).astype(np.float32)
    dR = O.to_bf16_f32(rng.standard_normal((B, T, N, Hh, Dv)).astype(np.float32))
    dS = rng.standard_normal((B, Hh, Dk, Dv)).astype(np.float32)
    ref = _ref_grads(*(O.to_bf16_f32(x) for x in (q, k, v)), a, b, s0, dR, dS, 2, 3)
    got = _hip_grads(hip, q, k, v, a, b, s0, dR, dS, 2, 3, dtype=torch.bfloat16)
    for name, g, r in zip("q k v alpha beta s0".split(), got, ref):
        lim = 1e-4 * max(1.0, np.abs(r).max()) + (np.abs(r) * 2.0 ** -7 if name in "qkv" else 0)
        assert np.all(np.abs(g - r) <= lim), (name, np.abs(g - r).max())


def test_wide_key_delta_parallel_limit(hip):
    """delta_parallel trains at up to 64 tokens per frame (test_wide_key_scan_backward, rule 1) and is refused beyond, as at Dk = 64."""
    q, k, v, a, b = make_scan_inputs(1, 2, 100, 1, 128, 16, seed=13, normalized=False, logits=True)
    t = [torch.from_numpy(x).cuda().requires_grad_() for x in (q, k, v, a, b)]
    with pytest.raises(hip.GdkvmError, match="delta_parallel"):
        hip.scan(*t, None, 1, 3)


@pytest.mark.parametrize("N", [49, 100])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_wide_key_training_forward_is_the_inference_forward(hip, N, dtype):
    """The training forward's R and S_T are gdkvm_scan_fwd's bits (the same kernel, writing the history beside), and two backward calls
    on the same inputs give the same bits."""
    q, k, v, a, b = make_scan_inputs(2, 3, N, 2, 128, 32, seed=N, normalized=False, logits=True, corr=0.5)
    dev = lambda x, dt=torch.float32: torch.from_numpy(x).cuda().to(dt)
    s0 = 0.3 * torch.randn(2, 2, 128, 32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(N))
    R0, S0 = hip.scan_fwd(dev(q, dtype), dev(k, dtype), dev(v, dtype), dev(a), dev(b), s0, flags=3)
    dR = torch.randn(R0.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)).to(dtype)
    outs = []
    for _ in range(2):
        t = [dev(q, dtype).requires_grad_(), dev(k, dtype).requires_grad_(), dev(v, dtype).requires_grad_(), dev(a).requires_grad_(),
             dev(b).requires_grad_(), s0.clone().requires_grad_()]
        R, S = hip.scan(*t, 2, 3)
        torch.autograd.backward([R, S], [dR, torch.ones_like(S)])
        outs.append([R, S] + [x.grad for x in t])
    assert torch.equal(outs[0][0], R0) and torch.equal(outs[0][1], S0)
    for x, y in zip(*outs):
        assert torch.equal(x, y)


@pytest.mark.parametrize("size", [64, 160])
def test_wide_key_module_gradients_match_the_independent_restatement(hip, size):
    """key_dim = value_dim = 128: module gradients against oracle.model_plain.plain_loss_and_grads, at 16 tokens per frame and at 100
    (beyond 64: the route of the Dk = 64 chunked training path)."""
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    from gdkvm_amd.train import segmentation_loss_lowres
    from oracle.model_plain import plain_loss_and_grads
    cfg = GDKVMConfig(key_dim=128, value_dim=128, widths=(16, 32, 64), pixel_dim=64)
    torch.manual_seed(4)
    model = GDKVM(cfg).train()
    g = torch.Generator().manual_seed(12)
    frames = torch.rand(2, 3, 3, size, size, generator=g)
    target = (torch.rand(2, 3, size, size, generator=g) > 0.5).long()
    target[0, 0, :9] = 255
    sd = {k_: v_.detach().cpu().clone() for k_, v_ in model.state_dict().items()}
    lp, gp = plain_loss_and_grads(sd, frames, target, key_dim=128, value_dim=128)
    model = model.cuda().to(memory_format=torch.channels_last)
    loss = segmentation_loss_lowres(model(frames.cuda(), _lowres=True), target.cuda())
    loss.backward()
    assert abs(loss.item() - lp.item()) <= 2e-4 * max(1.0, abs(lp.item())), (loss.item(), lp.item())
    seen = 0
    for n, p in model.named_parameters():
        if n not in gp:
            continue
        scale = max(gp[n].abs().max().item(), 1e-6)
        err = (p.grad.double().cpu() - gp[n]).abs().max().item() / scale
        assert err <= 2e-3, (n, err, scale)
        seen += 1
    assert seen >= 60


def test_wide_key_graphed_training_step(hip):
    """The default widths at key_dim = value_dim = 128, bf16: the captured step replays the eager step's bits, two runs from the same
    start agree bit for bit, and the loss falls over a short fit."""
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    from gdkvm_amd.train import GraphedTrainStep, fit_synthetic, train_step
    from tests.test_train_side_gpu import _ellipse_batches
    cfg = GDKVMConfig(key_dim=128, value_dim=128)
    steps = 3
    frames, target = _ellipse_batches(steps + 1, 2, 4, 112, 61)

    def run(graph):
        torch.manual_seed(62)
        model = GDKVM(cfg).cuda().train().to(memory_format=torch.channels_last)
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3, fused=True, capturable=True)
        if graph:
            step = GraphedTrainStep(model, opt, frames[0], target[0], torch.bfloat16, warmup=2)
            losses = [step(frames[i], target[i]).item() for i in range(1, steps + 1)]
        else:
            for _ in range(2):
                train_step(model, opt, frames[0], target[0], torch.bfloat16)
            losses = [train_step(model, opt, frames[i], target[i], torch.bfloat16).item() for i in range(1, steps + 1)]
        return losses, {n: p.detach().clone() for n, p in model.named_parameters()}

    le, we = run(False)
    le2, we2 = run(False)
    lg, wg = run(True)
    assert le == le2 and all(torch.equal(we[n], we2[n]) for n in we), (le, le2)
    assert le == lg, (le, lg)
    for n in we:
        assert torch.equal(we[n], wg[n]), n

    torch.manual_seed(63)
    model = GDKVM(cfg).cuda().train().to(memory_format=torch.channels_last)
    losses = fit_synthetic(model, steps=12, clips=4, frames=4, size=112, seed=3)
    assert all(np.isfinite(losses)) and np.mean(losses[-3:]) < np.mean(losses[:3]) - 0.05, losses
