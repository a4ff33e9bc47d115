"""Whole-module parity on the GPU: GDKVM (torch convs + HIP memory path) vs GDKVMRef (torch CPU convs + oracle)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _pair(cfg=None, seed=0):
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    from oracle.model_ref import GDKVMRef
    torch.manual_seed(seed)
    cfg = cfg or GDKVMConfig()
    ref = GDKVMRef(cfg).eval()
    ref.math = "f64"
    for m in ref.modules():                      # non-trivial BatchNorm statistics
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.8, 1.25)
    model = GDKVM(cfg).eval()
    model.load_state_dict(ref.state_dict())
    return ref, model.cuda().to(memory_format=torch.channels_last)


def _balance(ref, model, frames):
    """Random init puts one class everywhere; shift the head bias by the median logit gap so masks are mixed."""
    with torch.no_grad():
        lg = ref(frames)
        for c in range(1, lg.shape[2]):
            gap = (lg[:, :, 0] - lg[:, :, c]).median()
            ref.decoder.head.bias[c] += gap
            model.decoder.head.bias[c] += gap.to(model.decoder.head.bias.device)


def test_module_fp32_matches_cpu_reference(hip):
    ref, model = _pair()
    frames = torch.rand(2, 4, 3, 112, 112)
    _balance(ref, model, frames)
    with torch.no_grad():
        lr, sr = ref(frames, return_state=True)
        lg, sg = model(frames.cuda(), return_state=True)
    lg = lg.cpu(); sg = sg.cpu()
    assert (lg - lr).abs().max() <= 1e-3 and (sg - sr).abs().max() <= 1e-3
    mr, mg = lr.argmax(2), lg.argmax(2)
    frac = mr.float().mean().item()
    assert 0.2 < frac < 0.8, f"degenerate mask ({frac})"
    disagree = (mr != mg)
    # every disagreeing pixel must be a near-tie of the reference logits (MIOpen vs MKLDNN summation order)
    margin = (lr[:, :, 0] - lr[:, :, 1]).abs()
    assert disagree.float().mean() <= 1e-3 and (margin[disagree] <= 1e-3).all()


def test_module_against_the_independent_restatement(hip):
    """The product on the GPU -- fp32 module, and the fused bf16 inference build -- against oracle/model_plain.plain_forward, which
    shares no code with gdkvm_amd (float64, torch.nn.functional + the numpy oracle, from the state_dict alone): layer wiring included."""
    from oracle.model_plain import plain_forward
    ref, model = _pair(seed=4)
    frames = torch.rand(2, 3, 3, 112, 112)
    _balance(ref, model, frames)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    lp, sp = plain_forward(sd, frames)
    with torch.no_grad():
        lg, sg = model(frames.cuda(), return_state=True)
    assert (lg.cpu().double() - lp).abs().max() <= 1e-3 and (sg.cpu().double() - sp).abs().max() <= 1e-3
    frac = lp.argmax(2).float().mean().item()
    assert 0.2 < frac < 0.8, f"degenerate mask ({frac})"
    with torch.no_grad():
        fused = model.fuse_for_inference().to(torch.bfloat16)
        lb = fused(frames.cuda()).float().cpu().double()
    err = (lb - lp).abs()
    rms = lp.pow(2).mean().sqrt().item()                # errors relative to the logits' own scale (random-init logits are small)
    # (mean relative to the logits' rms; the largest single error by the tighter of the rms-relative bound and the absolute one the test
    #  used before -- for logits of rms >= 1 a 30 %-of-rms outlier would otherwise pass)
    assert err.mean() <= 0.05 * rms and err.max() <= min(0.3 * rms, 0.05 * max(1.0, lp.abs().max().item())), (err.max().item() / rms, err.mean().item() / rms)
    agree = (lb.argmax(2) == lp.argmax(2)).float().mean().item()
    assert agree >= 0.97, agree


def test_module_with_keys_wider_than_64(hip):
    """key_dim = 128 (one head; KPFF's LDS tile bounds Cp + Hh (Dk + Dv) at the default's 576): the module's inference path on the general scan kernel (csrc/gdr_general.hip) -- fp32 module and fused
    bf16 build against oracle/model_plain.plain_forward run at the same widths; the state keeps its [B, Hh, 128, Dv] shape across calls."""
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    from oracle.model_plain import plain_forward
    torch.manual_seed(31)
    cfg = GDKVMConfig(heads=1, key_dim=128, value_dim=128)
    model = GDKVM(cfg).eval()
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.8, 1.25)
    frames = torch.rand(2, 3, 3, 112, 112)
    sd = {k_: v_.detach().clone() for k_, v_ in model.state_dict().items()}
    lp, _ = plain_forward(sd, frames, heads=1, key_dim=128, value_dim=128)
    with torch.no_grad():                               # balance the random-init head so that both classes appear
        model.decoder.head.bias -= lp.flatten(3).median(-1).values.mean((0, 1)).float()
    sd = {k_: v_.detach().clone() for k_, v_ in model.state_dict().items()}
    lp, sp = plain_forward(sd, frames, heads=1, key_dim=128, value_dim=128)
    model = model.cuda().to(memory_format=torch.channels_last)
    with torch.no_grad():
        lg, sg = model(frames.cuda(), return_state=True)
        la, sa = model(frames[:, :2].cuda(), return_state=True)
        lb2, sb = model(frames[:, 2:].cuda(), state=sa, return_state=True)
    assert tuple(sg.shape) == (2, 1, 128, 128)
    assert (lg.cpu().double() - lp).abs().max() <= 1e-3 and (sg.cpu().double() - sp).abs().max() <= 1e-3
    # the state carried across calls (fp32 module: the library convolutions of the encoder pick algorithms by batch size)
    assert (sb - sg).abs().max() <= 1e-4 and (torch.cat([la, lb2], 1) - lg).abs().max() <= 1e-4
    with torch.no_grad():
        fused = model.fuse_for_inference().to(torch.bfloat16)
        fb = frames.cuda().bfloat16()
        lbd, sbd = fused(fb, return_state=True)
        l1, s1 = fused(fb[:, :2], return_state=True)
        l2, s2 = fused(fb[:, 2:], state=s1, return_state=True)
        lb = lbd.float().cpu().double()
    assert torch.equal(s2, sbd) and torch.equal(torch.cat([l1, l2], 1), lbd)               # fused build: every kernel deterministic -> the same bits
    err = (lb - lp).abs()
    rms = lp.pow(2).mean().sqrt().item()
    assert err.mean() <= 0.05 * rms and err.max() <= 0.3 * rms, (err.max().item() / rms, err.mean().item() / rms)
    assert (lb.argmax(2) == lp.argmax(2)).float().mean().item() >= 0.95


def test_segment_captured_in_a_graph(hip):
    """GDKVM.graphed_segment: segment() of the fused bf16 build captured into a hipGraph and replayed == the eager call, bit for bit (masks
    and Dice counts), for the captured batch and for fresh batches copied into its input buffers; another shape is refused."""
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    torch.manual_seed(41)
    model = GDKVM(GDKVMConfig()).eval().fuse_for_inference().cuda().to(torch.bfloat16).to(memory_format=torch.channels_last)
    frames = [torch.rand(2, 4, 3, 112, 112, device="cuda").bfloat16() for _ in range(3)]
    target = [(torch.rand(2, 4, 112, 112, device="cuda") > 0.5).to(torch.uint8) for _ in range(3)]
    with torch.no_grad():
        want = [tuple(t.clone() for t in model.segment(f, t_)) for f, t_ in zip(frames, target)]
        g = model.graphed_segment(frames[0].clone(), target[0].clone())
        for f, t_, (m, c) in zip(frames, target, want):
            gm, gc = g(f, t_)
            assert torch.equal(gm, m) and torch.equal(gc, c)
        g2 = model.graphed_segment(frames[1])                  # without a target: masks only
        assert g2(frames[2])[1] is None and torch.equal(g2(frames[2])[0], want[2][0])
    with pytest.raises(RuntimeError):
        g(frames[0][:, :2], target[0][:, :2])


def test_segment_graph_with_the_batch_on_several_streams(hip):
    """GraphedSegment(streams=n): the batch as n equal groups of clips on n streams of ONE hipGraph, every group writing its slice of the one
    result -- the same masks and Dice counts as the eager call over the whole batch, bit for bit (clips never interact); 8 clips default to
    two streams; fresh batches go through the input buffers; groups that do not divide the batch are refused; the state-carrying form splits the state with the clips."""
    from gdkvm_amd.model import GDKVM, GDKVMConfig, GraphedSegment
    torch.manual_seed(43)
    model = GDKVM(GDKVMConfig()).eval().fuse_for_inference().cuda().to(torch.bfloat16).to(memory_format=torch.channels_last)
    frames = [torch.rand(8, 3, 3, 112, 112, device="cuda").bfloat16() for _ in range(2)]
    target = [(torch.rand(8, 3, 112, 112, device="cuda") > 0.5).to(torch.uint8) for _ in range(2)]
    with torch.no_grad():
        want = [tuple(t.clone() for t in model.segment(f, t_)) for f, t_ in zip(frames, target)]
        g = model.graphed_segment(frames[0].clone(), target[0].clone())
        assert g.streams == 2
        for n in (2, 4):
            gn = GraphedSegment(model, frames[0].clone(), target[0].clone(), streams=n)
            for f, t_, (m, c) in zip(frames, target, want):
                gm, gc = gn(f, t_)
                assert gm.shape == m.shape and torch.equal(gm, m) and torch.equal(gc, c), n
        gm, gc = g(frames[1], target[1])
        assert torch.equal(gm, want[1][0]) and torch.equal(gc, want[1][1])
        g1 = GraphedSegment(model, frames[0].clone(), streams=2)                 # without a target: masks only
        assert g1(frames[1])[1] is None and torch.equal(g1(frames[1])[0], want[1][0])
        with pytest.raises(ValueError):
            GraphedSegment(model, frames[0].clone(), streams=3)
        # the state-carrying form on two streams: masks, counts and the final state of segment(..., state=, return_state=True)
        s0 = 0.3 * torch.randn(8, 1, 64, 256, device="cuda")
        wm, wc, ws = model.segment(frames[1], target[1], state=s0, return_state=True)
        gs = GraphedSegment(model, frames[0].clone(), target[0].clone(), state=torch.zeros_like(s0), streams=2)
        gm, gc, gst = gs(frames[1], target[1], state=s0)
        assert torch.equal(gm, wm) and torch.equal(gc, wc) and torch.equal(gst, ws)


def test_fused_build_on_maps_wider_than_64_pixels(hip):
    """528x528 frames: the stride-8 map is 66 pixels wide, wider than the chunked 3x3 kernel tiles -- those layers and the strided ones
    take the general implicit-GEMM kernel; 33x33 = 1089 tokens per frame.  The fused bf16 build against the independent restatement."""
    from oracle.model_plain import plain_forward
    ref, model = _pair(seed=6)
    frames = torch.rand(1, 2, 3, 528, 528)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    lp, _ = plain_forward(sd, frames, lowres=True)
    gap = (lp[:, :, 0] - lp[:, :, 1]).median()                    # balance the two classes (as _balance does, on the restatement)
    sd["decoder.head.bias"][1] += gap.float()
    lp[:, :, 1] += gap
    with torch.no_grad():
        model.decoder.head.bias[1] += gap.float().cuda()
        fused = model.fuse_for_inference().to(torch.bfloat16)
        lb = fused(frames.cuda(), _lowres=True).float().cpu().double()
    err = (lb - lp).abs()
    rms = lp.pow(2).mean().sqrt().item()
    # (mean relative to the logits' rms; the largest single error by the tighter of the rms-relative bound and the absolute one the test
    #  used before -- for logits of rms >= 1 a 30 %-of-rms outlier would otherwise pass)
    assert err.mean() <= 0.05 * rms and err.max() <= min(0.3 * rms, 0.05 * max(1.0, lp.abs().max().item())), (err.max().item() / rms, err.mean().item() / rms)
    agree = (lb.argmax(2) == lp.argmax(2)).float().mean().item()
    frac = lp.argmax(2).float().mean().item()
    assert agree >= 0.97 and 0.2 < frac < 0.8, (agree, frac)


def test_module_fp32_on_a_grid_wider_than_16_tokens(hip):
    """320x320 frames: a 20x20 token grid (400 tokens per frame: chunked scan, KPFF tiles of 4 rows x 16 columns)."""
    ref, model = _pair(seed=3)
    frames = torch.rand(1, 2, 3, 320, 320)
    _balance(ref, model, frames)
    with torch.no_grad():
        lr, sr = ref(frames, return_state=True)
        lg, sg = model(frames.cuda(), return_state=True)
    lg = lg.cpu(); sg = sg.cpu()
    assert (lg - lr).abs().max() <= 1e-3 and (sg - sr).abs().max() <= 1e-3
    mr, mg = lr.argmax(2), lg.argmax(2)
    margin = (lr[:, :, 0] - lr[:, :, 1]).abs()
    disagree = (mr != mg)
    assert disagree.float().mean() <= 1e-3 and (margin[disagree] <= 1e-3).all()


def test_module_state_carry_and_mask0(hip):
    ref, model = _pair(seed=1)
    frames = torch.rand(1, 6, 3, 112, 112).cuda()
    mask0 = (torch.rand(1, 1, 112, 112) > 0.5).float().cuda()
    with torch.no_grad():
        full, s_full = model(frames, mask0=mask0, return_state=True)
        a, s = model(frames[:, :2], mask0=mask0, return_state=True)
        b, s2 = model(frames[:, 2:], state=s, return_state=True)
    # the memory path is bit-identical under chunking (tests/test_scan_gpu.py); the MIOpen convs around it may pick
    # another algorithm for another batch size, so the module as a whole is compared with a tolerance
    assert (torch.cat([a, b], 1) - full).abs().max() <= 1e-4 and (s2 - s_full).abs().max() <= 1e-4
    with torch.no_grad():
        other = model(frames, mask0=1 - mask0)
    assert not torch.equal(other, full)           # the first-frame mask does reach the memory


def test_module_bf16_fused_dice_parity(hip):
    """bf16 inference build (BatchNorm folded, bf16 conv weights) vs the fp32 CPU reference: Dice of the masks."""
    from gdkvm_amd import ops
    ref, model = _pair(seed=2)
    frames = torch.rand(2, 8, 3, 112, 112)
    _balance(ref, model, frames)
    with torch.no_grad():
        mr, _ = ref.segment(frames)
        model = model.fuse_for_inference().to(torch.bfloat16)
        assert model.kpff.wa.dtype == torch.float32          # KPFF weights stay fp32 under .to(bfloat16)
        mg, counts = model.segment(frames.cuda(), target=mr.cuda())
    dice = ops.dice_from_counts(counts.sum((0, 1))).cpu().numpy()
    assert (dice >= 0.97).all(), dice
    assert 0.2 < mr.float().mean() < 0.8


def test_invalidate_packed_weights_reaches_the_fused_convolutions(hip):
    """An in-place write through .data changes neither the version counter nor the address the weight packs are keyed on:
    invalidate_packed_weights() must drop every FusedConv's fragment-ordered copy too, or the convolution kernels keep reading
    the old weights."""
    from gdkvm_amd.model import FusedConv
    _, model = _pair(seed=5)
    frames = torch.rand(1, 2, 3, 112, 112).cuda().bfloat16()
    with torch.no_grad():
        model = model.fuse_for_inference().to(torch.bfloat16)
        before = model(frames, _lowres=True).float()
        conv = model.encoder.layer2[1].conv1                       # a 128 -> 128 layer on the packed-weight kernel
        assert isinstance(conv, FusedConv) and conv in model._packs.slots
        conv.conv.weight.data.mul_(0)
        stale = model(frames, _lowres=True).float()
        assert torch.equal(stale, before)                          # (the hazard: the pack is still the old weights)
        model.invalidate_packed_weights()
        assert conv not in model._packs.slots and conv.__dict__["_packs"] is model._packs
        after = model(frames, _lowres=True).float()
    assert not torch.equal(after, before)


def test_module_gradients_match_cpu_reference(hip):
    """One training step's gradients: GDKVM (MIOpen convs + HIP forward/backward kernels) vs GDKVMRef (CPU convs +
    autograd through the fp64 torch restatement), same weights, same batch, train-mode BatchNorm."""
    from gdkvm_amd.model import GDKVMConfig
    from gdkvm_amd.train import segmentation_loss
    cfg = GDKVMConfig(widths=(16, 32, 64), pixel_dim=64, value_dim=64)
    ref, model = _pair(cfg, seed=3)
    ref.train(); model.train()
    frames = torch.rand(2, 3, 3, 64, 64)
    target = (torch.rand(2, 3, 64, 64) > 0.5).long()
    segmentation_loss(ref(frames), target).backward()
    segmentation_loss(model(frames.cuda()), target.cuda()).backward()
    worst = 0.0
    for (n, pr), (_, pg) in zip(ref.named_parameters(), model.named_parameters()):
        if pr.grad is None:
            assert pg.grad is None or pg.grad.abs().max() == 0, n
            continue
        scale = max(pr.grad.abs().max().item(), 1e-6)
        err = (pg.grad.cpu() - pr.grad).abs().max().item() / scale
        worst = max(worst, err)
        assert err <= 2e-3, (n, err, scale)
    assert worst > 0


def test_module_gradients_match_the_independent_restatement(hip):
    """The same step against oracle.model_plain.plain_loss_and_grads -- architecture, objective and ignore-label rule written a second
    time in float64 from the state_dict alone, nothing shared with gdkvm_amd -- for the host loss on full-resolution logits AND for the
    fused objective of train_step (stride-4 logits into gdkvm_seg_loss_fwd / _bwd), with unlabelled pixels in the batch."""
    from gdkvm_amd.model import GDKVMConfig
    from gdkvm_amd.train import segmentation_loss, segmentation_loss_lowres
    from oracle.model_plain import plain_loss_and_grads
    cfg = GDKVMConfig(widths=(16, 32, 64), pixel_dim=64, value_dim=64)
    _, model = _pair(cfg, seed=4)
    model.train()
    g = torch.Generator().manual_seed(12)
    frames = torch.rand(2, 3, 3, 64, 64, generator=g)
    target = (torch.rand(2, 3, 64, 64, generator=g) > 0.5).long()
    target[:, 2] = 255                                                          # a whole unlabelled frame (EchoNet clips: most of them)
    target[0, 0, :9] = 255
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    lp, gp = plain_loss_and_grads(sd, frames, target, value_dim=64)
    for fused in (False, True):
        model.zero_grad(set_to_none=True)
        if fused:
            loss = segmentation_loss_lowres(model(frames.cuda(), _lowres=True), target.cuda())
        else:
            loss = segmentation_loss(model(frames.cuda()), target.cuda())
        loss.backward()
        assert abs(loss.item() - lp.item()) <= 2e-4 * max(1.0, abs(lp.item())), (fused, loss.item(), lp.item())
        seen = 0
        for n, p in model.named_parameters():
            if n not in gp:
                assert p.grad is None or p.grad.abs().max() == 0, n
                continue
            scale = max(gp[n].abs().max().item(), 1e-6)
            err = (p.grad.double().cpu() - gp[n]).abs().max().item() / scale
            assert err <= 2e-3, (fused, n, err, scale)
            seen += 1
        assert seen >= 60


def test_train_and_eval_entry_points(hip, tmp_path):
    """Row n2 smoke: a few optimisation steps through train.py (HIP forward + backward kernels), a checkpoint, then eval.py
    on it; the loss must drop and the evaluation must print per-class Dice."""
    import json
    import subprocess
    import sys
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["data.size=64", "data.frames=4", "data.num_classes=2", "batch_size=4", f"run_dir={tmp_path}", "log_every=5",
              "model.value_dim=64"]
    out = subprocess.run([sys.executable, os.path.join(root, "train.py"), "num_iterations=30", "save_every=30", "learning_rate=1e-3"] + common,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    losses = [float(l.split("loss")[1].split()[0]) for l in out.stdout.splitlines() if l.startswith("step")]
    assert len(losses) == 6 and losses[-1] < losses[0], losses
    # the entry point runs the step in the form the benchmark measures: one hipGraph replay (GraphedTrainStep, fused AdamW), not the eager loop
    how = [l for l in out.stdout.splitlines() if l.startswith("train step:")]
    assert how and "GraphedTrainStep" in how[0] and "fused" in how[0], out.stdout[-1500:]
    assert "not captured" not in out.stderr
    ck = os.path.join(tmp_path, "gdkvm_step30.pth")
    assert os.path.exists(ck)
    ev = subprocess.run([sys.executable, os.path.join(root, "eval.py"), "--weights", ck, "eval_stage.num_vis=1"] + common,
                        capture_output=True, text=True, timeout=600)
    assert ev.returncode == 0, ev.stderr[-2000:]
    res = json.loads(ev.stdout.strip().splitlines()[-1])
    assert len(res["dice_per_class"]) == 2 and 0.0 <= res["mean_foreground_dice"] <= 1.0
    assert res["forward"]["graph_replays"] >= 6 and res["forward"]["eager_calls"] <= 2, res     # GraphedSegment per batch shape (first sight: eager)
    assert "not captured" not in ev.stderr
    # the eager forms stay reachable and agree: same Dice from the un-captured forward
    ev2 = subprocess.run([sys.executable, os.path.join(root, "eval.py"), "--weights", ck] + common, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, GDKVM_FWD_GRAPH="0"))
    assert ev2.returncode == 0, ev2.stderr[-2000:]
    res2 = json.loads(ev2.stdout.strip().splitlines()[-1])
    assert res2["dice_per_class"] == res["dice_per_class"] and res2["forward"]["graph_replays"] == 0
    assert os.listdir(os.path.join(tmp_path, "vis"))


def test_bench_plain_run_times_its_steps_and_dumps_the_masks(hip, tmp_path):
    """bench.py without --full: ONE JSON line carrying the headline alone, --steps timed steps, `ms_per_step` consistent with `value`;
    --dump-outputs writes the last timed step's masks (float32 class indices of a balanced head: both classes present), and a second run
    with the same arguments writes the same masks (seeded inputs and weights)."""
    import json
    import subprocess
    import sys
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    masks = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, p.stdout[-2000:]
        out = json.loads(lines[0])
        assert out["steps"] == 3 and out["warmup"] == 1 and out["unit"] == "frames/s" and out["dtype"] == "bf16"
        assert out["ms_per_step"] > 0 and abs(16 * 32 / (out["ms_per_step"] * 1e-3) / out["value"] - 1) < 0.01, out
        assert not {"roofline", "cpu_baseline", "train_step", "pipeline", "step_mode"} & set(out), sorted(out)
        assert sorted(os.listdir(d)) == ["masks.npy"]
        masks.append(np.load(d / "masks.npy"))
    m = masks[0]
    assert m.dtype == np.float32 and m.shape == (16, 32, 112, 112) and m.nbytes <= 64e6
    assert set(np.unique(m).tolist()) == {0.0, 1.0} and 0.05 < m.mean() < 0.95, m.mean()
    assert np.array_equal(masks[0], masks[1])


def test_dice_parity_on_a_fitted_model(hip):
    """BASELINE.json's second figure of merit, "Dice vs reference", on a model whose head separates the classes by real margins: a short fit
    on the synthetic echo clips (the training step itself: HIP forward / backward kernels, fused loss, AdamW), then on held-out clips
    (a) the fp32 module on the GPU against the CPU reference module (torch CPU convolutions + the fp64 oracle memory path) with the SAME
    weights, (b) the fused bf16 inference build against the fp32 module, (c) both against the labels.  With a random-init head the bf16
    build agrees on 97-98 % of the pixels because logits differ by ~1e-3 everywhere; fitted, the masks coincide except on the contour."""
    from gdkvm_amd import ops, train
    from gdkvm_amd.data import SyntheticEchoClips
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    from oracle.model_ref import GDKVMRef
    torch.manual_seed(21)
    cfg = GDKVMConfig()
    model = GDKVM(cfg).cuda().to(memory_format=torch.channels_last)
    losses = train.fit_synthetic(model, steps=60, clips=8, frames=8, size=112, seed=5)
    assert losses[-1] < 0.5 * losses[0], (losses[0], losses[-1])
    held = SyntheticEchoClips(4, 8, 112, 2, seed=99)
    x = torch.stack([held[i][0] for i in range(4)])
    y = torch.stack([held[i][1] for i in range(4)]).to(torch.uint8)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    ref = GDKVMRef(cfg).eval()
    ref.load_state_dict(sd)
    with torch.no_grad():
        m_ref, _ = ref.segment(x[:2])
        m32, c32 = model.segment(x.cuda(), target=y.cuda())
        fused = GDKVM(cfg).eval()
        fused.load_state_dict(sd)
        fused = fused.cuda().to(memory_format=torch.channels_last).fuse_for_inference().to(torch.bfloat16)
        m16, c16 = fused.segment(x.cuda(), target=m32)
        _, c16y = fused.segment(x.cuda(), target=y.cuda())
    d_label32 = ops.dice_from_counts(c32.sum((0, 1)))[1].item()
    d_label16 = ops.dice_from_counts(c16y.sum((0, 1)))[1].item()
    d_16_vs_32 = ops.dice_from_counts(c16.sum((0, 1)))[1].item()
    agree_ref = (m32[:2].cpu() == m_ref).float().mean().item()
    fg = (m32 == 1).float().mean().item()
    print(f"fitted model: loss {losses[0]:.3f} -> {losses[-1]:.3f}; foreground {fg:.3f}; Dice vs labels fp32 {d_label32:.4f} / bf16 {d_label16:.4f}; "
          f"bf16 build vs fp32 module {d_16_vs_32:.4f}; fp32 GPU vs CPU reference mask agreement {agree_ref:.5f}")
    assert 0.02 < fg < 0.6
    assert d_label32 >= 0.8 and d_label16 >= 0.8                  # it learned the cavity
    assert agree_ref >= 0.9995                                    # GPU module == CPU reference module, same weights (measured: 1.00000)
    assert d_16_vs_32 >= 0.998                                    # bf16 inference build against the fp32 module (measured: 0.9997 - 0.9999)


def test_device_prefetcher_delivers_every_batch_in_order(hip):
    """gdkvm_amd.pipeline.DevicePrefetcher (what train.py / eval.py iterate): batches arrive on the device in order and intact -- from plain
    host tensors (staged through the prefetcher's own pinned buffers) and from already pinned ones (copied straight from them), with two and
    three slots, uint8 frames scaled to [0, 1] in the requested dtype, integer targets cast; more batches than slots, a short last batch."""
    from gdkvm_amd.pipeline import DevicePrefetcher
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(3)
    batches = [(torch.randint(0, 256, (3 if i < 6 else 2, 4, 3, 16, 16), generator=g, dtype=torch.uint8),
                torch.randint(0, 4, (3 if i < 6 else 2, 4, 16, 16), generator=g)) for i in range(7)]
    for pinned, threaded in ((False, True), (True, True), (False, False), (True, False)):
        for slots in (2, 3):
            src = [(f.pin_memory(), t.pin_memory()) for f, t in batches] if pinned else batches
            pre = DevicePrefetcher(iter(src), dev, slots=slots, frames_dtype=torch.bfloat16, target_dtype=torch.uint8, threaded=threaded)
            got = []
            for f, t in pre:
                assert f.is_cuda and f.dtype == torch.bfloat16 and t.dtype == torch.uint8
                got.append((f.float().cpu().clone(), t.cpu().clone()))      # (valid until the next next(): copied here)
                torch.cuda.current_stream().synchronize()
            assert len(got) == len(batches) and pre.h2d_bytes == sum(f.numel() + 8 * t.numel() for f, t in batches)
            for (f, t), (f0, t0) in zip(got, batches):
                assert torch.equal(t, t0.to(torch.uint8))
                assert torch.equal(f, (f0.to(torch.bfloat16) * (1.0 / 255.0)).float())
    # only the frames need a cast (the target already has its dtype), over more batches than slots
    mixed = [(torch.randint(0, 256, (2, 2, 3, 8, 8), generator=g, dtype=torch.uint8), torch.randint(0, 2, (2, 2, 8, 8), generator=g, dtype=torch.uint8)) for _ in range(5)]
    seen = [(f.float().cpu().clone(), t.cpu().clone()) for f, t in DevicePrefetcher(mixed, dev, slots=2, frames_dtype=torch.bfloat16)]
    assert all(torch.equal(f, (f0.to(torch.bfloat16) * (1.0 / 255.0)).float()) and torch.equal(t, t0) for (f, t), (f0, t0) in zip(seen, mixed))
    float_batches = [(torch.rand(2, 2, 3, 8, 8, generator=g), torch.zeros(2, 2, 8, 8, dtype=torch.long)) for _ in range(3)]
    def broken():                                             # an exception inside the loader reaches the consumer (threaded: from the worker)
        yield float_batches[0]
        raise ValueError("loader broke")
    for threaded in (True, False):
        with pytest.raises(ValueError, match="loader broke"):
            for _ in DevicePrefetcher(broken(), dev, threaded=threaded):
                pass
    early = iter(DevicePrefetcher(float_batches, dev, threaded=True))       # a consumer that stops early leaves no worker behind
    next(early)
    early.close()
    out = [f.clone() for f, _ in DevicePrefetcher(float_batches, dev)]
    assert all(o.dtype == torch.float32 and torch.equal(o.cpu(), f) for o, (f, _) in zip(out, float_batches))


def test_graphed_segments_sharing_one_memory_pool(hip):
    """Several GraphedSegment captures over DIFFERENT input buffers in ONE memory pool (bench.py rotates eight input batches this way: the
    activations of every replay live at the same addresses, nothing is copied in the timed region): replayed in turn, each graph returns
    the masks of ITS batch, bit-equal to the eager forward; one and two streams inside."""
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    torch.manual_seed(13)
    model = GDKVM(GDKVMConfig()).cuda().eval().to(memory_format=torch.channels_last)
    batches = [torch.rand(8, 3, 3, 112, 112, device="cuda").bfloat16() for _ in range(3)]
    with torch.no_grad():                                     # (a random-init head puts one class everywhere: balance it, so that the batches' masks differ)
        lg = model(batches[0].float(), _lowres=True)
        model.decoder.head.bias[1] += (lg[:, :, 0] - lg[:, :, 1]).median()
    model = model.fuse_for_inference().to(torch.bfloat16)
    want = [model.segment(b)[0].clone() for b in batches]
    assert not torch.equal(want[0], want[1]) and 0.1 < (want[0] != 0).float().mean().item() < 0.9
    for streams in (1, 2):
        graphs = []
        for b in batches:
            graphs.append(model.graphed_segment(b, streams=streams, pool=None if not graphs else graphs[0].graph.pool()))
        for rnd in range(2):
            for i in (2, 0, 1):
                assert torch.equal(graphs[i](batches[i])[0], want[i]), (streams, rnd, i)


def test_forwards_in_flight_return_every_batch_s_masks(hip):
    """model.InFlightSegments (bench.py's timed loop: graphs replayed in turn on two host streams, step i + 1 starting while step i runs) and
    pipeline.SegmentRunner(in_flight=2) with results collected one batch behind (eval.py's loop): every batch's masks and Dice counts are the
    eager forward's, bit for bit, under back-to-back launches; in_flight = 1 and direct calls give the same."""
    from gdkvm_amd.model import GDKVM, GDKVMConfig, InFlightSegments
    from gdkvm_amd.pipeline import SegmentRunner
    torch.manual_seed(29)
    model = GDKVM(GDKVMConfig()).cuda().eval().to(memory_format=torch.channels_last)
    batches = [torch.rand(8, 3, 3, 112, 112, device="cuda").bfloat16() for _ in range(4)]
    targets = [(torch.rand(8, 3, 112, 112, device="cuda") > 0.5).to(torch.uint8) for _ in range(4)]
    with torch.no_grad():
        lg = model(batches[0].float(), _lowres=True)
        model.decoder.head.bias[1] += (lg[:, :, 0] - lg[:, :, 1]).median()
    model = model.fuse_for_inference().to(torch.bfloat16)
    want = [tuple(t.clone() for t in model.segment(b, target=t_)) for b, t_ in zip(batches, targets)]
    assert not torch.equal(want[0][0], want[1][0])
    ring = InFlightSegments(model, batches, targets, in_flight=2)
    outs = []
    for rnd in range(3):
        for i in range(4):
            outs.append((i, ring.launch(i)))                   # no waiting between launches: two forwards overlap
        ring.synchronize()
        for i, (m, c, _) in outs[-4:]:
            assert torch.equal(m, want[i][0]) and torch.equal(c, want[i][1]), (rnd, i)
    ring.launch(1)
    ring.wait(1)                                               # the caller's stream waits for that replay only
    assert torch.equal(ring.graphs[1].out[0].clone(), want[1][0])
    with pytest.raises(ValueError):
        InFlightSegments(model, batches[:3], in_flight=2)
    for in_flight in (2, 1):
        runner = SegmentRunner(model, min_repeats=1, in_flight=in_flight)
        got, pending = [], None
        for rnd in range(2):
            for b, t_ in zip(batches, targets):
                nxt = runner.submit(b, t_)
                if pending is not None:
                    got.append(pending.get())
                pending = nxt
        got.append(pending.get())
        torch.cuda.synchronize()
        assert len(got) == 8 and runner.eager_calls == 0
        for k, (m, c) in enumerate(got):
            assert torch.equal(m, want[k % 4][0]) and torch.equal(c, want[k % 4][1]), (in_flight, k)
        m, c = runner(batches[2], targets[2])
        assert torch.equal(m, want[2][0]) and torch.equal(c, want[2][1])


def test_graph_replays_zero_the_dice_counts_every_time(hip):
    """The Dice counts are accumulated with integer atomics from zero.  Regression (round 6): their zeroing was a hipMemsetAsync, and as a
    memset node of a captured graph over a counts tensor inside the graph's own memory pool it ran on the first replay only -- the single-stream
    GraphedSegment with a target returned wrong counts from the second replay on.  It is a kernel now (csrc/gdkvm_api.hip gdkvm_zero_async):
    four replays of the one- and the two-stream graph all equal the eager forward's counts; so does the bare entry point captured by itself."""
    from gdkvm_amd import ops
    from gdkvm_amd.model import GDKVM, GDKVMConfig, GraphedSegment
    torch.manual_seed(31)
    model = GDKVM(GDKVMConfig()).cuda().eval().to(memory_format=torch.channels_last)
    b = torch.rand(8, 3, 3, 112, 112, device="cuda").bfloat16()
    t = (torch.rand(8, 3, 112, 112, device="cuda") > 0.5).to(torch.uint8)
    with torch.no_grad():
        lg = model(b.float(), _lowres=True)
        model.decoder.head.bias[1] += (lg[:, :, 0] - lg[:, :, 1]).median()
    model = model.fuse_for_inference().to(torch.bfloat16)
    want_m, want_c = (x.clone() for x in model.segment(b, target=t)[:2])
    assert want_c.sum().item() > 0
    for streams in (1, 2):
        g = GraphedSegment(model, b, t, streams=streams)
        for r in range(4):
            m, c = g(b, t)[:2]
            assert torch.equal(m, want_m) and torch.equal(c, want_c), (streams, r)
    logits = torch.randn(6, 2, 112, 112, device="cuda")
    target = (torch.rand(6, 112, 112, device="cuda") > 0.5).to(torch.uint8)
    ref = ops.argmax_dice(logits, target)[1].clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.argmax_dice(logits, target)[1]               # (the counts tensor is allocated INSIDE the capture: the graph's pool)
    for r in range(4):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref), r


def test_full_size_forward_clips_are_independent(hip):
    """configs[1] at its full size (16 clips x 32 frames x 112 x 112, bf16, the fused inference build): clips never interact, so the forward over
    the whole batch equals the forwards over any split of it BIT FOR BIT -- stride-4 logits and masks -- although the kernels' grids, tile walks
    and launch forms change with the batch (5 + 1 + 10 clips against 16).  The property the clip sharding over GPUs (distributed.shard_range)
    and the graph's groups of clips rest on."""
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    torch.manual_seed(7)
    model = GDKVM(GDKVMConfig()).cuda().eval().to(memory_format=torch.channels_last)
    x = torch.rand(16, 32, 3, 112, 112, device="cuda").bfloat16()
    with torch.no_grad():
        lg = model(x[:4].float(), _lowres=True)
        model.decoder.head.bias[1] += (lg[:, :, 0] - lg[:, :, 1]).median()
    model = model.fuse_for_inference().to(torch.bfloat16)
    with torch.no_grad():
        full = model.segment(x)[0].clone()
        assert 0.1 < (full != 0).float().mean().item() < 0.9
        parts = torch.cat([model.segment(x[a:b].contiguous())[0].clone() for a, b in ((0, 5), (5, 6), (6, 16))])
        assert torch.equal(full, parts)
        lo = model(x, _lowres=True).clone()
        lo_parts = torch.cat([model(x[a:b].contiguous(), _lowres=True).clone() for a, b in ((0, 5), (5, 16))])
        assert torch.equal(lo, lo_parts)
