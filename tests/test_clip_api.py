"""The host side of gradient clipping (mm2d3d_amd/clip.py): argument handling that needs no GPU."""
import pytest
import torch


def test_parse_clip_takes_lightning_s_names_and_defaults():
    from mm2d3d_amd.clip import parse_clip

    assert parse_clip(None) is None and parse_clip(("norm", None)) is None and parse_clip(("value", None)) is None
    assert parse_clip(0.5) == ("norm", 0.5) and parse_clip(("value", 2)) == ("value", 2.0) and parse_clip(["norm", 1]) == ("norm", 1.0)
    for bad in (("l1", 1.0), ("", 1.0), ("norm", -1.0), ("value", float("nan"))):
        with pytest.raises(ValueError):
            parse_clip(bad)


def test_trainer_reads_gradient_clip_val_and_algorithm():
    from mm2d3d_amd.train import TrainModel

    mods = lambda: {"2d_net": torch.nn.Linear(2, 2), "3d_net": torch.nn.Linear(2, 2)}
    assert TrainModel(mods(), None, None, {})._clip is None
    assert TrainModel(mods(), None, None, {"gradient_clip_algorithm": "value"})._clip is None  # no value: off, as in Lightning
    assert TrainModel(mods(), None, None, {"gradient_clip_val": 0.5})._clip == ("norm", 0.5)
    assert TrainModel(mods(), None, None, {"gradient_clip_val": 0.5, "gradient_clip_algorithm": "value"})._clip == ("value", 0.5)
    with pytest.raises(ValueError):
        TrainModel(mods(), None, None, {"gradient_clip_val": 0.5, "gradient_clip_algorithm": "l1"})


def test_clip_functions_refuse_other_optimizers_norm_types_and_cpu_arenas():
    from mm2d3d_amd.clip import clip_grad_norm_, clip_grad_value_
    from mm2d3d_amd.optimizers import FlatSGD

    plain = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=1.0)
    with pytest.raises(TypeError):
        clip_grad_norm_(plain, 1.0)
    with pytest.raises(TypeError):
        clip_grad_value_([plain], 1.0)
    flat = FlatSGD([torch.nn.Parameter(torch.zeros(3))], lr=1.0)
    for bad in (1, float("inf"), 2.5):
        with pytest.raises(NotImplementedError):
            clip_grad_norm_(flat, 1.0, norm_type=bad)
    with pytest.raises(RuntimeError):  # the clip is a HIP kernel: no CPU fallback
        clip_grad_norm_(flat, 1.0)
