"""Training in the per-frame step mode (GDKVMConfig(mask_feedback=True)): the weight-gradient kernel of the mask embedding
(gdkvm_mask_embed_wgrad), the module's two-pass training forward against an independent CPU reference, the buffers the feedback pass must
leave alone, the default-width bf16 step eager and as one graph, and the train.py / eval.py entry points."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import gdkvm_oracle as O

pytestmark = pytest.mark.gpu


def _masks(F, H, W, ncls, seed):
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(0, ncls, (F, H, W), generator=g, dtype=torch.uint8)
    m[torch.rand(F, H, W, generator=g) < 0.1] = 255                      # unlabelled pixels count as background
    m[: max(1, F // 4), : H // 3] = 0                                    # some all-background cells
    m[F // 2:, H // 2:, : W // 2] = 1                                    # and all-foreground ones
    return m


def _wgrad_ref(m, dv, h, w):
    mn = m.numpy()
    pooled = O.mask_cell_mean((mn != 0) & (mn != 255), h, w)            # [F, N] float64
    return np.einsum("fn,fnc->c", pooled, dv.double().numpy())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("geom", [(6, 112, 112, 7, 7, 256, 2), (3, 256, 256, 16, 16, 256, 2), (5, 120, 88, 8, 6, 64, 4),
                                  (5, 120, 88, 7, 6, 64, 4), (4, 64, 64, 4, 4, 1024, 4), (512, 112, 112, 7, 7, 256, 2),
                                  (512, 256, 256, 16, 16, 64, 2)])
def test_mask_embed_wgrad_matches_fp64_and_repeats(hip, dtype, geom):
    """d_w[c] = sum over frames and tokens of mean_cell(m != 0, n) * d_v'[f, n, c] against the fp64 einsum of the oracle's pooling: 112^2 to 7x7,
    256^2 to 16x16, 120x88 cells ragged in width and in both directions, four classes with 255 pixels, 512 frames -- at 256^2 that is
    131 072 token rows, four 64-row chunks per block; two runs are bit-identical."""
    F, H, W, h, w, C, ncls = geom
    m = _masks(F, H, W, ncls, seed=F + H + C)
    dv = torch.randn(F, h * w, C, generator=torch.Generator().manual_seed(C + F)).to(dtype)
    ref = _wgrad_ref(m, dv, h, w)                                         # (bf16: the stored values, exactly)
    got = hip.mask_embed_wgrad(m.cuda(), dv.cuda(), h, w)
    again = hip.mask_embed_wgrad(m.cuda(), dv.cuda(), h, w)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got.shape == (C,)
    err = np.abs(got.cpu().double().numpy() - ref).max() / np.abs(ref).max()
    assert err <= 1e-5, err
    assert torch.equal(got, again)
    if dtype == torch.bfloat16:                                           # against the unrounded fp32 gradient: the input's 2^-8
        dv32 = torch.randn(F, h * w, C, generator=torch.Generator().manual_seed(C + F))
        ref32 = _wgrad_ref(m, dv32, h, w)
        assert np.abs(got.cpu().double().numpy() - ref32).max() <= 2.0 ** -7 * np.abs(ref32).max() + 1e-3


def test_mask_embed_wgrad_arguments(hip):
    """A workspace below gdkvm_mask_embed_wgrad_workspace_bytes raises; no frame gives zeros; the autograd form's forward IS
    gdkvm_mask_embed_add (bit for bit) and its backward passes d_v' through unchanged."""
    F, H, W, h, w, C = 4, 112, 112, 7, 7, 64
    m = _masks(F, H, W, 2, seed=3).cuda()
    dv = torch.randn(F, h * w, C, device="cuda")
    need = int(hip.load().gdkvm_mask_embed_wgrad_workspace_bytes(F, h, w, C))
    assert need >= C * 4
    with pytest.raises(hip.GdkvmError):
        hip.mask_embed_wgrad(m, dv, h, w, workspace=torch.empty(need - 16, dtype=torch.uint8, device="cuda"))
    ok = hip.mask_embed_wgrad(m, dv, h, w, workspace=torch.empty(need, dtype=torch.uint8, device="cuda"))
    assert torch.equal(ok, hip.mask_embed_wgrad(m, dv, h, w))
    assert torch.equal(hip.mask_embed_wgrad(m[:0], dv[:0], h, w), torch.zeros(C, device="cuda"))
    for dtype in (torch.float32, torch.bfloat16):
        v = torch.randn(F, h * w, C, device="cuda").to(dtype).requires_grad_()
        wt = torch.randn(C, 1, 1, 1, device="cuda", requires_grad=True)
        out = hip.mask_embed(v, m, wt, h, w)
        plain = hip.mask_embed_add_(v.detach().clone(), m, wt.detach().reshape(-1).contiguous(), h, w)
        assert torch.equal(out.detach(), plain)
        g = torch.randn_like(out)
        out.backward(g)
        assert torch.equal(v.grad, g)
        assert torch.equal(wt.grad.reshape(-1), hip.mask_embed_wgrad(m, g, h, w))


def _fed_ref_class():
    from oracle.model_ref import GDKVMRef

    class FedRef(GDKVMRef):
        """GDKVMRef (CPU convolutions, fp64 autograd memory path) with the embedding of GIVEN masks added to every frame's values inside
        _project: the step mode's recurrence with the masks held fixed, written without the product's kernels."""
        fed = None                  # uint8 [B,T,H,W]
        skip0 = False               # frame 0 carries mask0's embedding instead

        def _project(self, f16, B, T, mask0=None):
            p, k, q, v, a, b, n = super()._project(f16, B, T, mask0)
            if self.fed is None:
                return p, k, q, v, a, b, n
            h, w = f16.shape[-2:]
            m = self.fed.reshape(B * T, *self.fed.shape[-2:]).numpy()
            pooled = torch.from_numpy(O.mask_cell_mean((m != 0) & (m != 255), h, w)).reshape(B, T, h * w)
            if self.skip0:
                pooled[:, 0] = 0.0
            e = pooled.to(v.dtype)[..., None] * self.mask_embed.weight.reshape(-1)
            return p, k, q, v + e.reshape(v.shape), a, b, n

    return FedRef


def _small_pair(seed):
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    cfg = GDKVMConfig(widths=(16, 32, 64), pixel_dim=64, value_dim=64, mask_feedback=True)
    torch.manual_seed(seed)
    ref = _fed_ref_class()(dataclasses.replace(cfg, mask_feedback=False)).train()
    ref.math = "f64"
    with torch.no_grad():
        ref.mask_embed.weight.mul_(4.0)                                   # make the fed-back masks matter
    model = GDKVM(cfg).train()
    return cfg, ref, model


def _mix_head(ref, frames, **kw):
    """shift the head bias so that the masks are mixed (a random-init head puts one class on every pixel)"""
    with torch.no_grad():
        lr = ref(frames, _lowres=True, **kw)
        ref.decoder.head.bias[1] += (lr[:, :, 0] - lr[:, :, 1]).median()


@pytest.mark.parametrize("case", [(2, 4, False), (2, 4, True), (1, 4, False), (1, 3, True), (2, 1, False), (3, 1, True)])
def test_feedback_training_gradients_match_the_cpu_reference(hip, case):
    """fp32, small widths, B clips x T frames (one clip; single-frame clips too), one frame unlabelled where there are several: loss and every
    parameter gradient of the two-pass training forward against GDKVMRef fed the product's own fed-back masks -- mask_embed.weight among
    them, and nonzero -- with and without a first-frame mask."""
    from gdkvm_amd.train import segmentation_loss
    B, T, with_mask0 = case
    cfg, ref, model = _small_pair(seed=31 + 7 * B + T + int(with_mask0))
    g = torch.Generator().manual_seed(7)
    frames = torch.rand(B, T, 3, 64, 64, generator=g)
    target = (torch.rand(B, T, 64, 64, generator=g) > 0.5).long()
    if T > 2:
        target[:, 2] = 255
    mask0 = None
    if with_mask0:
        mask0 = torch.zeros(B, 1, 64, 64)
        mask0[:, :, 16:44, 20:50] = 1.0
    _mix_head(ref, frames, mask0=mask0)
    model.load_state_dict(ref.state_dict())
    model = model.cuda().to(memory_format=torch.channels_last)
    logits, s_out, masks = model(frames.cuda(), mask0=None if mask0 is None else mask0.cuda(), return_state=True, return_masks=True)
    assert masks.dtype == torch.uint8 and masks.shape == (B, T, 64, 64)
    fg = (masks != 0).float().mean().item()
    assert 0.02 < fg < 0.98, fg
    loss = segmentation_loss(logits, target.cuda())
    loss.backward()
    ref.fed, ref.skip0 = masks.cpu(), mask0 is not None
    logits_r, s_ref = ref(frames, mask0=mask0, return_state=True)
    lr_ = segmentation_loss(logits_r, target)
    lr_.backward()
    assert abs(loss.item() - lr_.item()) <= 2e-4 * max(1.0, abs(lr_.item())), (loss.item(), lr_.item())
    # the state after the last frame carries every frame's embedding, the last frame's too (which no read-out sees): v + e, not more
    s_err = (s_out.detach().cpu().double() - s_ref.detach().double()).abs().max().item()
    assert s_err <= 1e-3 * max(1.0, s_ref.abs().max().item()), s_err
    seen = 0
    for (n, pr), (_, pg) in zip(ref.named_parameters(), model.named_parameters()):
        if pr.grad is None:
            assert pg.grad is None or pg.grad.abs().max() == 0, n
            continue
        scale = max(pr.grad.abs().max().item(), 1e-6)
        err = (pg.grad.cpu().double() - pr.grad.double()).abs().max().item() / scale
        assert err <= 2e-3, (n, err, scale)
        seen += 1
    assert seen >= 60
    if T > 1:
        assert ref.mask_embed.weight.grad is not None and ref.mask_embed.weight.grad.abs().max().item() > 0     # (compared above)
        assert model.mask_embed.weight.grad.abs().max().item() > 0
    else:                               # one frame: its write reaches only the final state, no read-out -- the loss cannot see the embedding
        assert model.mask_embed.weight.grad is not None and model.mask_embed.weight.grad.abs().max().item() == 0


def test_fed_back_masks_are_the_reference_feedback_loop(hip):
    """Pass 1's masks against GDKVMRef's own per-frame loop (_forward_feedback, train mode, no_grad, fp64 memory path): equal wherever the
    reference margin between the two largest logits exceeds the tolerance."""
    import torch.nn.functional as F
    cfg, ref, model = _small_pair(seed=33)
    frames = torch.rand(2, 4, 3, 64, 64, generator=torch.Generator().manual_seed(8))
    _mix_head(ref, frames)
    model.load_state_dict(ref.state_dict())
    model = model.cuda().to(memory_format=torch.channels_last)
    _, masks = model(frames.cuda(), return_masks=True)
    with torch.no_grad():
        low, rm, _, _ = ref._forward_feedback(frames, None, None, lowres=True)
    full = F.interpolate(low.flatten(0, 1).double(), size=(64, 64), mode="bilinear", align_corners=False)
    top = full.topk(2, dim=1).values
    margin = (top[:, 0] - top[:, 1]).reshape(2, 4, 64, 64)
    decided = margin > 2e-3
    assert decided.float().mean().item() > 0.5
    fg = (rm != 0).float().mean().item()
    assert 0.02 < fg < 0.98, fg
    assert torch.equal(masks.cpu()[decided], rm[decided])


def _bn_buffers(model):
    return {n: b.detach().clone() for n, b in model.named_buffers()
            if any(n.endswith(s) for s in ("running_mean", "running_var", "num_batches_tracked"))}


def _default_model(seed):
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    torch.manual_seed(seed)
    return GDKVM(GDKVMConfig(mask_feedback=True)).cuda().train().to(memory_format=torch.channels_last)


def test_feedback_pass_writes_no_buffer(hip):
    """Default widths, bf16: the feedback pass leaves every BatchNorm buffer bit-identical; the whole training forward bumps every
    num_batches_tracked exactly once and moves the running statistics (pass 2)."""
    model = _default_model(41)
    frames = torch.rand(2, 4, 3, 112, 112, device="cuda")
    seen = []
    inner = model._feedback_pass

    def watched(*a, **kw):
        before = _bn_buffers(model)
        out = inner(*a, **kw)
        after = _bn_buffers(model)
        seen.append(all(torch.equal(before[n], after[n]) for n in before))
        return out

    model._feedback_pass = watched
    b0 = _bn_buffers(model)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        logits, masks = model(frames, _lowres=True, return_masks=True)
    b1 = _bn_buffers(model)
    assert seen == [True]
    nbt = [n for n in b0 if n.endswith("num_batches_tracked")]
    assert len(nbt) >= 19
    for n in nbt:
        assert int(b1[n]) == int(b0[n]) + 1, n
    assert all(not torch.equal(b0[n], b1[n]) for n in b0 if n.endswith("running_mean"))
    assert logits.shape == (2, 4, 2, 28, 28) and masks.shape == (2, 4, 112, 112)


def _blob_batches(n, B, T, size, seed):
    """frames whose bright ellipse is the label: a batch the model can learn"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(size), torch.arange(size), indexing="ij")
    fr, tg = [], []
    for _ in range(n):
        c = torch.rand(B, T, 2, generator=g) * size * 0.4 + size * 0.3
        r = torch.rand(B, T, 1, generator=g) * size * 0.1 + size * 0.15
        inside = ((yy - c[..., :1, None]) ** 2 + (xx - c[..., 1:, None]) ** 2) < r[..., None] ** 2
        f = 0.3 * torch.rand(B, T, 3, size, size, generator=g) + 0.6 * inside[:, :, None].float()
        fr.append(f.cuda())
        tg.append(inside.long().cuda())
    return fr, tg


@pytest.fixture
def strict(monkeypatch):
    import gdkvm_amd.model
    monkeypatch.setattr(gdkvm_amd.model, "_STRICT", True)


def test_feedback_train_step_eager_graph_and_repeat(hip, strict):
    """Default widths, bf16, 2 x 4 x 112^2, library fallbacks fatal: train_step runs; GraphedTrainStep equals the eager step bit for bit
    over 3 steps (losses and weights); two identical eager runs are bit-identical."""
    from gdkvm_amd.train import GraphedTrainStep, train_step
    frames, target = _blob_batches(4, 2, 4, 112, 51)

    def run(graph):
        model = _default_model(52)
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3, fused=True, capturable=True)
        if graph:
            step = GraphedTrainStep(model, opt, frames[0], target[0], torch.bfloat16, warmup=1)
            losses = [step(frames[i], target[i]).item() for i in range(1, 4)]
        else:
            train_step(model, opt, frames[0], target[0], torch.bfloat16)
            losses = [train_step(model, opt, frames[i], target[i], torch.bfloat16).item() for i in range(1, 4)]
        torch.cuda.synchronize()
        return losses, {n: p.detach().clone() for n, p in model.named_parameters()}, _bn_buffers(model)

    le, we, be = run(False)
    le2, we2, be2 = run(False)
    lg, wg, bg = run(True)
    assert all(np.isfinite(le))
    assert le == le2 and le == lg, (le, le2, lg)
    for n in we:
        assert torch.equal(we[n], we2[n]) and torch.equal(we[n], wg[n]), n
    for n in be:
        assert torch.equal(be[n], be2[n]) and torch.equal(be[n], bg[n]), n


def _fg_dice(mask, target):
    p, t = mask == 1, target == 1
    return (2 * (p & t).sum() / (p.sum() + t.sum()).clamp_min(1)).item()


def test_feedback_training_learns_and_infers(hip, strict):
    """About 20 steps on a learnable batch: the loss falls and mask_embed.weight moves; the trained model then segments a batch it has not
    seen in step-mode inference (fused bf16 build): foreground Dice, not pixel agreement, as the ellipses cover ~12 % of the pixels."""
    from gdkvm_amd.train import train_step
    steps = 20
    frames, target = _blob_batches(steps + 1, 2, 4, 112, 61)
    model = _default_model(62)
    opt = torch.optim.AdamW(model.parameters(), lr=2e-3, fused=True, capturable=True)
    w0 = model.mask_embed.weight.detach().clone()
    losses = [train_step(model, opt, frames[i], target[i], torch.bfloat16).item() for i in range(steps)]
    assert np.mean(losses[-4:]) < np.mean(losses[:4]) - 0.1, losses
    assert (model.mask_embed.weight.detach() - w0).abs().max().item() > 1e-3
    fm = model.eval().fuse_for_inference().to(torch.bfloat16).to(memory_format=torch.channels_last)
    with torch.no_grad():
        mk, _ = fm.segment(frames[steps].bfloat16())
    assert mk.shape == (2, 4, 112, 112) and mk.dtype == torch.uint8
    dice = _fg_dice(mk, target[steps])
    print("held-out foreground Dice", dice, "losses", losses)
    assert dice > 0.5, dice


def test_feedback_train_and_eval_entry_points(hip, tmp_path):
    """train.py with model.mask_feedback=true for a few steps, then eval.py on the checkpoint in the step mode: the loss drops and per-class
    Dice is printed."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["data.size=64", "data.frames=4", "data.num_classes=2", "batch_size=4", f"run_dir={tmp_path}", "log_every=5",
              "model.value_dim=64", "model.mask_feedback=true"]
    out = subprocess.run([sys.executable, os.path.join(root, "train.py"), "num_iterations=30", "save_every=30", "learning_rate=1e-3"] + common,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    losses = [float(l.split("loss")[1].split()[0]) for l in out.stdout.splitlines() if l.startswith("step")]
    assert len(losses) == 6 and losses[-1] < losses[0], losses
    ck = os.path.join(tmp_path, "gdkvm_step30.pth")
    assert os.path.exists(ck)
    ev = subprocess.run([sys.executable, os.path.join(root, "eval.py"), "--weights", ck] + common, capture_output=True, text=True, timeout=600)
    assert ev.returncode == 0, ev.stderr[-2000:]
    res = json.loads(ev.stdout.strip().splitlines()[-1])
    assert len(res["dice_per_class"]) == 2 and 0.0 <= res["mean_foreground_dice"] <= 1.0
