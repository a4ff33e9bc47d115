"""The machinery of tests/test_train_trace_gpu.py on the CPU: its wiring table and its float64 per-call references, chained call by call
from the frames to the loss (forward node by node, then each node's vector-Jacobian product sent back along the table), reproduce
oracle.model_plain.plain_loss_and_grads -- the architecture and objective written down independently -- at the default widths.  A
failure of the GPU test then points at the product, not at the table or the references."""
import pytest
import torch

from tests import train_trace as TT


def _model(cfg, seed):
    from gdkvm_amd.model import GDKVM
    torch.manual_seed(seed)
    m = GDKVM(cfg)
    for mod in m.modules():                      # non-trivial BatchNorm affine parameters
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.weight.data.uniform_(0.8, 1.2); mod.bias.data.normal_(0, 0.1)
    return m


@pytest.mark.parametrize("shape,ncls", [((2, 3, 112, 112), 2), ((2, 3, 120, 88), 4)])
def test_per_call_references_chained_along_the_wiring_equal_the_plain_restatement(shape, ncls):
    from gdkvm_amd.model import GDKVMConfig
    from oracle.model_plain import plain_loss_and_grads
    cfg = GDKVMConfig(num_classes=ncls)
    sd = _model(cfg, seed=3).state_dict()
    B, T, H, W = shape
    g = torch.Generator().manual_seed(8)
    frames = torch.rand(B, T, 3, H, W, generator=g)
    target = torch.randint(0, ncls, (B, T, H, W), generator=g)
    target[:, 1, : H // 3] = 255                                               # unlabelled pixels
    loss, grads = TT.chain(cfg, sd, frames, target)
    lp, gp = plain_loss_and_grads(sd, frames, target, heads=cfg.heads, key_dim=cfg.key_dim, value_dim=cfg.value_dim, rule=cfg.rule)
    assert abs(loss.item() - lp.item()) <= 1e-10 * abs(lp.item())
    assert set(grads) == set(gp), sorted(set(grads) ^ set(gp))
    for n in gp:
        err = (grads[n] - gp[n]).abs().max().item()
        assert err <= 1e-10 * gp[n].abs().max().item(), (n, err)


def test_wiring_covers_the_default_architecture():
    """Every parameter of the default model except mask_embed (no first-frame mask in a training step) enters exactly one node; the
    node list holds each entry point the number of times the architecture implies."""
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    cfg = GDKVMConfig()
    nodes = TT.wiring(cfg, 2, 3, 112, 112)
    used = [p for n in nodes for p in n.params.values()]
    assert len(used) == len(set(used))
    names = {n for n, _ in GDKVM(cfg).named_parameters()}
    assert set(used) == names - {"mask_embed.weight"}
    counts = {}
    for n in nodes:
        counts[n.entry] = counts.get(n.entry, 0) + 1
    assert counts == TT.CENSUS


@pytest.mark.parametrize("entry", ["bn_act", "bn_relu_pool", "conv3x3_fork", "seg_loss"])
def test_teacher_forced_references_keep_the_derivative(entry):
    """reference(bf16=True) rounds where the kernels round and takes the ReLU mask from the recorded output; on values that are already
    bf16 numbers, with the mask the forward itself produces, its vector-Jacobian product is the plain one (torch autograd, float64): the
    teacher forcing changes no derivative."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(len(entry))
    bfv = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).to(torch.bfloat16).to(torch.float64)
    x, w, b = bfv(3, 16, 9, 7), 1 + 0.2 * bfv(16), 0.1 * bfv(16)
    if entry == "bn_act":
        res = bfv(3, 16, 9, 7)
        args = [x, w, b, None, None, res, 0.1, 1e-5, True]
        plain = lambda x, w, b, res: F.relu(F.batch_norm(x, None, None, w, b, True, 0.0, 1e-5) + res)
        leaves = [x, w, b, res]
        mask = plain(x, w, b, res) > 0
    elif entry == "bn_relu_pool":
        args = [x, w, b, None, None, 0.1, 1e-5]
        plain = lambda x, w, b: F.max_pool2d(F.relu(F.batch_norm(x, None, None, w, b, True, 0.0, 1e-5)), 3, 2, 1)
        leaves = [x, w, b]
        mask = None
    elif entry == "conv3x3_fork":
        wt = bfv(8, 16, 3, 3)
        args = [x, wt]
        plain = lambda x, wt: (F.conv2d(x, wt, None, 1, 1) ** 2).sum() + (x ** 3).sum()      # conv output and skip both reach it
        leaves = [x, wt]
        mask = None
    else:
        from oracle.model_plain import plain_objective
        z = bfv(2, 3, 5, 4)
        tg = torch.randint(0, 3, (2, 20, 16), generator=g)
        tg[0, :4] = 255
        args = [z, tg, 1.0, 1.0]
        plain = lambda z: plain_objective(F.interpolate(z, size=(20, 16), mode="bilinear", align_corners=False).unsqueeze(0), tg.unsqueeze(0))
        leaves = [z]
        mask = None
    leaves = [t.clone().requires_grad_() for t in leaves]
    it = iter(leaves)
    a = [next(it) if isinstance(v, torch.Tensor) and v.is_floating_point() else v for v in args]
    outs = TT.reference(entry, a, bf16=True, relu_mask=mask)
    if entry == "conv3x3_fork":
        dys = {0: 2 * F.conv2d(leaves[0], leaves[1], None, 1, 1).detach(), 1: 3 * leaves[0].detach() ** 2}
    elif entry == "bn_relu_pool":                # (gradients whose sums over the <= 4 windows of an element are bf16 numbers again)
        dys = {0: torch.randint(-4, 5, outs[0].shape, generator=g).to(torch.float64) / 8}
    else:
        dys = {0: torch.ones_like(outs[0]) if outs[0].dim() == 0 else bfv(*outs[0].shape)}
    got = TT.vjp(outs, dys, leaves)
    p_leaves = [t.detach().clone().requires_grad_() for t in leaves]
    y = plain(*p_leaves)
    if entry == "conv3x3_fork":
        want = torch.autograd.grad(y, p_leaves)
    else:
        want = torch.autograd.grad(y, p_leaves, dys[0])
    for a_, b_ in zip(got, want):
        assert (a_ - b_).abs().max().item() <= 1e-12 * max(1.0, b_.abs().max().item())
