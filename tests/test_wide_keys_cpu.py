"""The key width per head reaches the model from the run configuration (train.py / eval.py)."""
from gdkvm_amd.config import load_config


def test_key_dim_override():
    cfg = load_config(None, ["model.key_dim=128"])
    assert cfg.model.key_dim == 128
    assert load_config(None, []).model.key_dim == 64
