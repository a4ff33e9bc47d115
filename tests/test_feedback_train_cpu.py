"""The step mode's training surface on the CPU: configuration, the C ABI entry point of the mask-embedding weight gradient, and the
forward's argument checks (the kernels themselves: tests/test_feedback_train_gpu.py)."""
import os

import pytest
import torch


def test_model_cfg_carries_mask_feedback(tmp_path):
    from gdkvm_amd.config import ModelCfg, load_config
    assert ModelCfg().mask_feedback is False
    assert load_config(None, ["model.mask_feedback=true"]).model.mask_feedback is True
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = load_config(os.path.join(root, "config", "config_gdkvm_01.yaml"))
    assert cfg.model.mask_feedback is False


def test_mask_embed_wgrad_is_declared_and_bound():
    from gdkvm_amd import ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "gdkvm.h")) as f:
        hdr = f.read()
    for name in ("gdkvm_mask_embed_wgrad", "gdkvm_mask_embed_wgrad_workspace_bytes"):
        assert name + "(" in hdr and name in ops.SIGNATURES


def test_mask_embed_wgrad_workspace_bytes():
    """One fp32 partial row of C columns per block, about 512 blocks over the F*h*w token rows."""
    from gdkvm_amd import build, ops
    build.build()
    lib = ops.load()
    assert lib.gdkvm_mask_embed_wgrad_workspace_bytes(16 * 32, 7, 7, 256) == 512 * 256 * 4
    assert lib.gdkvm_mask_embed_wgrad_workspace_bytes(1, 2, 2, 64) == 4 * 64 * 4          # (fewer rows than blocks: one row each)
    assert lib.gdkvm_mask_embed_wgrad_workspace_bytes(0, 7, 7, 256) == 0


def test_return_masks_needs_the_step_mode():
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    model = GDKVM(GDKVMConfig(widths=(16, 32, 64), pixel_dim=64, value_dim=64))
    with pytest.raises(ValueError, match="return_masks"):
        model(torch.rand(1, 2, 3, 64, 64), return_masks=True)


def test_step_mode_training_forward_is_not_refused_on_the_cpu_it_needs_the_gpu():
    """The training forward in the step mode runs the two passes (no NotImplementedError); the product has no CPU path, so on CPU tensors it
    stops at the first HIP kernel with GdkvmError."""
    from gdkvm_amd import ops
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    model = GDKVM(GDKVMConfig(widths=(16, 32, 64), pixel_dim=64, value_dim=64, mask_feedback=True)).train()
    with pytest.raises(ops.GdkvmError):
        model(torch.rand(1, 2, 3, 64, 64))
