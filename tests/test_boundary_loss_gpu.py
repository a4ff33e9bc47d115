"""GPU checks of the boundary loss: ops.signed_distance bit for bit against the restated definition (tests/boundary_reference.py) in both
kernel forms, ops.seg_loss_boundary (value, L_B and gradient) against the fp64 restatement at the project's loss cases, determinism, and the
training step with and without the term.  Tolerances are those of test_train_side_gpu.py::test_fused_objective_matches_the_torch_loss."""
import numpy as np
import pytest
import torch

from tests import boundary_reference as B
from tests import grid_caps as gc

pytestmark = pytest.mark.gpu

LDS_PIX = 79872                      # csrc/signed_distance.hip, SDM_LDS_PIX: frames of up to this many pixels live in LDS


def _labels(F, C, H, W, seed):
    return np.stack([B.label_frame(H, W, C, seed + f) for f in range(F)])


def _check_sd2(hip, t, C, classes=None):
    tg = torch.from_numpy(t).cuda()
    got = hip.signed_distance(tg, C, classes)
    assert got.dtype == torch.int32 and tuple(got.shape) == (t.shape[0], C) + t.shape[1:]
    want = B.sd2_reference(t, C)
    if classes is not None:
        keep = np.zeros(C, bool)
        keep[list(classes)] = True
        want = want * keep[None, :, None, None]
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want)
    assert torch.equal(got, hip.signed_distance(tg, C, classes))            # two calls are bit-equal
    return got


@pytest.mark.parametrize("shape", [(3, 4, 37, 53), (2, 2, 112, 112), (2, 3, 1, 40), (2, 3, 40, 1)])
def test_signed_distance_small_frames(hip, shape):
    """Odd sizes (H W no multiple of 16 or 32), 255s present, one-pixel-high and one-pixel-wide frames."""
    F, C, H, W = shape
    t = _labels(F, C, H, W, 10)
    assert (t == 255).any()
    _check_sd2(hip, t, C)
    off = np.concatenate([np.zeros(3, np.uint8), t.reshape(-1)])           # the frames at an odd byte address
    tg = torch.from_numpy(off).cuda()[3:].reshape(t.shape)
    assert tg.data_ptr() % 16 != 0
    assert np.array_equal(hip.signed_distance(tg, C).cpu().numpy().astype(np.int64), B.sd2_reference(t, C))


def test_signed_distance_at_256_with_a_corner_pixel(hip):
    """(2, 4, 256, 256), the 128 KiB plane of the LDS form; class 3 is a single corner pixel: sd2 reaches 2 * 255^2 = 130050."""
    t = _labels(2, 3, 256, 256, 20)
    t[0, 255, 255] = 3
    t[1, 0, 0] = 3
    got = _check_sd2(hip, t, 4)
    assert got[0, 3, 0, 0].item() == 130050 and got[0, 3, 255, 255].item() == -1 and got[1, 3, 255, 255].item() == 130050


@pytest.mark.parametrize("hw", [(256, 312), (256, 313), (313, 256)])
def test_signed_distance_on_both_sides_of_the_lds_bound(hip, hw):
    """256 x 312 = 79872 pixels is the largest LDS plane; 256 x 313 and 313 x 256 take the workspace form."""
    H, W = hw
    assert (H * W <= LDS_PIX) == (hw == (256, 312))
    need = hip._bytes("gdkvm_signed_distance_workspace_bytes", None, 1, 2, H, W)
    assert need == (0 if H * W <= LDS_PIX else 2 * 2 * ((H * W + 63) // 64 * 64))
    _check_sd2(hip, _labels(1, 2, H, W, 30), 2)


def test_signed_distance_absent_filling_masked_and_empty(hip):
    t = _labels(3, 4, 37, 53, 40)
    t[0][t[0] == 3] = 0                                                     # class 3 absent from frame 0
    t[1][:] = 1                                                             # class 1 fills frame 1
    t[2][:] = 255                                                           # no class at all in frame 2
    got = _check_sd2(hip, t, 4)
    assert not got[0, 3].any() and got[0, 2].any() and not got[1].any() and not got[2].any()
    only2 = _check_sd2(hip, t, 4, classes=[2])
    assert not only2[:, [0, 1, 3]].any() and only2[0, 2].any() and torch.equal(only2[:, 2], got[:, 2])
    assert _check_sd2(hip, t, 4, classes=[1, 0])[:, 1].any()
    e = hip.signed_distance(torch.empty(0, 37, 53, dtype=torch.uint8, device="cuda"), 4)
    assert tuple(e.shape) == (0, 4, 37, 53) and e.dtype == torch.int32
    long = torch.from_numpy(t).cuda().long()
    long[0, 0, 0], long[0, 0, 1] = 256, -1                                  # (a plain cast to uint8 would make them class 0 and 255)
    t2 = t.copy()
    t2[0, 0, 0] = t2[0, 0, 1] = 255
    assert np.array_equal(hip.signed_distance(long, 4).cpu().numpy().astype(np.int64), B.sd2_reference(t2, 4))
    with pytest.raises(hip.GdkvmError):
        hip.signed_distance(torch.from_numpy(t).cuda(), 4, classes=[4])
    with pytest.raises(hip.GdkvmError):
        hip.signed_distance(torch.from_numpy(t).cuda(), 4, classes=[1, 1])
    with pytest.raises(hip.GdkvmError):
        hip.signed_distance(torch.zeros(1, 4, 1025, dtype=torch.uint8, device="cuda"), 2)


LOSS_CASES = [(2, 3, 7, 5, 30, 17), (6, 2, 28, 28, 112, 112), (1, 8, 4, 4, 4, 4), gc.LOSS_CASE]
_REF = {}


def _loss_case(case, unlabelled):
    """Logits, labels (structured frames: a blob with a hole and scattered pixels, so that the distances are real), the reference's sd2."""
    key = (case, unlabelled)
    if key not in _REF:
        ni, c, h, w, H, W = case
        g = torch.Generator().manual_seed(sum(case))
        z = 2.0 * torch.randn(ni, c, h, w, generator=g)
        t = _labels(ni, c, H, W, sum(case))
        if unlabelled:
            t[(torch.rand(ni, H, W, generator=g) < 0.3).numpy()] = 255
        else:
            t[t == 255] = 0
        _REF[key] = (z, torch.from_numpy(t), B.sd2_reference(t, c), {})
    return _REF[key]


def _reference(case, unlabelled, dtype):
    """fp64 value, terms and gradient for the logits rounded to `dtype`, computed once per (case, dtype) and shared."""
    z, t, sd2, memo = _loss_case(case, unlabelled)
    if dtype not in memo:
        zb = z.to(dtype).double().requires_grad_(True)
        ref, ce, dice, lb = B.objective_lowres(zb, t, 0.7, 1.0, 0.05, None, sd2)
        (3.0 * ref).backward()
        memo[dtype] = (ref.item(), ce.item(), dice.item(), lb.item(), zb.grad)
    return memo[dtype]


@pytest.mark.parametrize("tdt", [torch.uint8, torch.int64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", LOSS_CASES)
def test_fused_boundary_objective(hip, case, dtype, tdt):
    """ops.seg_loss_boundary (weight 0.05, dice 0.7) against the fp64 restatement: value, out[3] = L_B and gradient; 30 % of the pixels are
    unlabelled in the grid-cap case (527 067 pixels: two trips of 2048 workgroups, eight partial rows per thread of the finalize)."""
    unlabelled = case == gc.LOSS_CASE
    z, t, _, _ = _loss_case(case, unlabelled)
    ref, ce, dice, lb, gref = _reference(case, unlabelled, dtype)
    za = z.to(dtype).cuda().requires_grad_(True)
    tg = t.cuda().to(tdt)
    loss, out = hip.seg_loss_boundary(za, tg, 0.7, 1.0, 0.05, terms=True)
    (3.0 * loss).backward()
    scale = gref.abs().max().item()
    gerr = (za.grad.double().cpu() - gref).abs().max().item()
    print("seg_loss_boundary", case, dtype, tdt, "loss", loss.item(), "ref", ref, "L_B", out[3].item(), "ref", lb, "grad err / scale", gerr / scale)
    assert abs(lb) > 1e-2 or case[2:] == (4, 4, 4, 4)
    assert abs(loss.item() - ref) <= 1e-5 * max(1.0, abs(ref))
    assert abs(out[3].item() - lb) <= 1e-5 * max(1.0, abs(lb))
    assert abs(out[1].item() - ce) <= 1e-5 * max(1.0, abs(ce)) and abs(out[2].item() - dice) <= 1e-5 and out[0].item() == loss.item()
    assert gerr <= (2.0 ** -7 if dtype == torch.bfloat16 else 1e-4) * scale
    # bit-equal over two calls, and from a signed distance map the caller made
    zb = z.to(dtype).cuda().requires_grad_(True)
    loss2, out2 = hip.seg_loss_boundary(zb, tg, 0.7, 1.0, 0.05, sd2=hip.signed_distance(tg, case[1]), terms=True)
    (3.0 * loss2).backward()
    assert torch.equal(out, out2) and torch.equal(za.grad, zb.grad)
    # weight 0: the entry agrees with ops.seg_loss
    plain = hip.seg_loss(z.to(dtype).cuda(), tg, 0.7, 1.0)
    zero = hip.seg_loss_boundary(z.to(dtype).cuda(), tg, 0.7, 1.0, 0.0)
    assert abs(zero.item() - plain.item()) <= 1e-5 * max(1.0, abs(plain.item()))


def test_fused_boundary_objective_classes_and_arguments(hip):
    """`classes` selects the planes (the others are not even computed), and bad arguments are refused on the host."""
    case = LOSS_CASES[0]
    z, t, sd2, _ = _loss_case(case, False)
    zb = z.double().requires_grad_(True)
    ref, _, _, lb = B.objective_lowres(zb, t, 0.7, 1.0, 0.05, [2, 0], sd2)
    ref.backward()
    za = z.cuda().requires_grad_(True)
    loss, out = hip.seg_loss_boundary(za, t.cuda(), 0.7, 1.0, 0.05, classes=[2, 0], terms=True)
    loss.backward()
    assert abs(loss.item() - ref.item()) <= 1e-5 * max(1.0, abs(ref.item())) and abs(out[3].item() - lb.item()) <= 1e-5 * max(1.0, abs(lb.item()))
    assert (za.grad.double().cpu() - zb.grad).abs().max() <= 1e-4 * zb.grad.abs().max()
    for kw in ({"classes": [3]}, {"classes": [1, 1]}, {"boundary_weight": -1.0}, {"boundary_weight": float("nan")},
               {"sd2": torch.zeros(2, 3, 30, 17, dtype=torch.int64, device="cuda")}, {"sd2": torch.zeros(2, 3, 30, 16, dtype=torch.int32, device="cuda")}):
        with pytest.raises(hip.GdkvmError):
            hip.seg_loss_boundary(z.cuda(), t.cuda(), 0.7, 1.0, **{"boundary_weight": 0.05, **kw})


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_boundary_objective_with_no_labelled_pixel(hip, dtype):
    z = (2.0 * torch.randn(3, 2, 28, 28, device="cuda")).to(dtype).requires_grad_(True)
    tg = torch.full((3, 112, 112), 255, dtype=torch.uint8, device="cuda")
    loss, out = hip.seg_loss_boundary(z, tg, 0.7, 1.0, 0.05, terms=True)
    loss.backward()
    assert torch.isfinite(out).all() and out[3].item() == 0.0 and torch.isfinite(z.grad).all()


def _small_model():
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    torch.manual_seed(11)
    return GDKVM(GDKVMConfig(widths=(16, 32, 64), pixel_dim=64, value_dim=64)).cuda().train().to(memory_format=torch.channels_last)


def test_train_step_at_weight_zero_launches_what_it_did(hip, monkeypatch):
    """With a spy on ops._call: at boundary_weight 0 the step calls gdkvm_seg_loss_fwd / _bwd and none of the new entry points; at 0.05 it calls
    the three new ones and not the old pair."""
    from gdkvm_amd.train import train_step
    frames = torch.rand(2, 3, 3, 64, 64, device="cuda")
    target = torch.from_numpy(_labels(6, 2, 64, 64, 50)).cuda().reshape(2, 3, 64, 64)
    names = []
    real = hip._call
    monkeypatch.setattr(hip, "_call", lambda name, *a: (names.append(name), real(name, *a))[1])
    new = {"gdkvm_signed_distance", "gdkvm_seg_loss_boundary_fwd", "gdkvm_seg_loss_boundary_bwd"}
    old = {"gdkvm_seg_loss_fwd", "gdkvm_seg_loss_bwd"}
    model = _small_model()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    train_step(model, opt, frames, target)
    plain = list(names)
    assert old <= set(plain) and not new & set(plain)
    del names[:]
    model = _small_model()
    train_step(model, torch.optim.AdamW(model.parameters(), lr=1e-3), frames, target, boundary_weight=0.0, boundary_classes=[1])
    assert names == plain                                                   # the same launches in the same order
    del names[:]
    model = _small_model()
    loss = train_step(model, torch.optim.AdamW(model.parameters(), lr=1e-3), frames, target, boundary_weight=0.05)
    assert new <= set(names) and not old & set(names) and torch.isfinite(loss)
    assert [n for n in names if n not in new] == [n for n in plain if n not in old]


def test_graphed_step_with_the_boundary_term(hip):
    """GraphedTrainStep at default widths, 2 clips x 2 frames x 64 x 64, bf16, weight 0.05: the replayed loss equals the eager step's from the
    same weights bit for bit, and differs from the weight-0 loss."""
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    from gdkvm_amd.train import GraphedTrainStep, train_step
    g = torch.Generator().manual_seed(3)
    frames = [torch.rand(2, 2, 3, 64, 64, generator=g).cuda() for _ in range(2)]
    target = [torch.from_numpy(_labels(4, 2, 64, 64, 60 + 4 * i)).cuda().long().reshape(2, 2, 64, 64) for i in range(2)]

    def run(graphed, weight):
        torch.manual_seed(22)
        model = GDKVM(GDKVMConfig()).cuda().train().to(memory_format=torch.channels_last)
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3, fused=True, capturable=True)
        kw = {"boundary_weight": weight} if weight else {}
        if graphed:
            step = GraphedTrainStep(model, opt, frames[0], target[0], torch.bfloat16, warmup=2, **kw)
            return step(frames[1], target[1]).item()
        for _ in range(2):
            train_step(model, opt, frames[0], target[0], torch.bfloat16, **kw)
        return train_step(model, opt, frames[1], target[1], torch.bfloat16, **kw).item()

    eager, replay, plain = run(False, 0.05), run(True, 0.05), run(True, 0.0)
    print("eager", eager, "replay", replay, "weight 0", plain)
    assert np.isfinite(eager) and eager == replay
    assert abs(replay - plain) > 1e-3
