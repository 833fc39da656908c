"""``train_kwargs["gradient_clip_val"]`` / ``["gradient_clip_algorithm"]`` of the trainer (Lightning's names, the reference's
run.py:262-288): one clipped ``fit_step`` on the smallest synthetic two-domain batch of tests/test_gpu_step.py, with SGD at a
learning rate under which the step IS the clipped gradient, without the loss scale (``"bf16"``) and with it (``16``)."""
import copy
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu

W = [1.9241476, 1.0, 2.16763851, 2.78254323, 1.54875664, 1.85686537]


def _nets(dev):
    from mm2d3d_amd.net2d import Net2DSeg
    from mm2d3d_amd.net3d import Net3DSeg

    torch.manual_seed(0)
    n2 = Net2DSeg(6, pretrained=False).to(dev)
    n3 = Net3DSeg(6, True, dict(in_channels=3, m=16, full_scale=4096, num_planes=7)).to(dev)
    for m in n2.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return n2, n3


def _trainer(dev, nets, lr, **train_kwargs):
    from mm2d3d_amd.losses import Loss
    from mm2d3d_amd.optimizers import Optimizer
    from mm2d3d_amd.train import TrainModel

    loss = Loss([{"name": "cross_entropy", "target": "segmentation", "args": {"weight": W}}])
    opts = {"2d_net": Optimizer("sgd", lr=lr), "3d_net": Optimizer("sgd", lr=lr)}
    tm = TrainModel({"2d_net": nets[0], "3d_net": nets[1]}, opts, loss,
                    dict(lambda_xm_src=1.0, lambda_xm_trg=0.1, gc_freeze=False, **train_kwargs))
    tm.configure_optimizers()
    return tm


def _batch(dev):
    from mm2d3d_amd.synthetic import make_batch

    return {"source": make_batch(5, 1, "nuscenes", (48, 64), device=dev), "target": make_batch(6, 1, "nuscenes", (48, 64), device=dev)}


def _weights(tm):
    return torch.cat([a["p"].double() for o in tm.optimizers for a in o._arenas if a is not None])


@pytest.mark.parametrize("precision", ["bf16", 16])
def test_one_fit_step_moves_the_weights_of_both_networks_by_the_clip_value_in_norm(precision):
    import mm2d3d_amd  # noqa: F401

    dev = torch.device("cuda:0")
    tm = _trainer(dev, _nets(dev), 1.0, precision=precision, gradient_clip_val=1e-3)
    assert bool(tm._scaler_cfg) == (precision == 16)
    w0 = _weights(tm)
    tm.fit_step(_batch(dev))
    dw = float((_weights(tm) - w0).norm())
    norm = float(tm.last_grad_norm)
    print(f"precision {precision}: gradient norm {norm!r}, |dw| {dw!r}")
    assert tm.last_grad_norm.device.type == "cuda"
    assert norm == norm and norm != float("inf") and norm > 1e-3
    assert abs(dw - 1e-3) <= 1e-4 * 1e-3
    if precision == 16:
        assert [tm.scaler.steps_taken(o) for o in tm.optimizers] == [1, 1]


@pytest.mark.parametrize("precision", ["bf16", 16])
def test_value_clipping_bounds_every_weight_s_move(precision):
    """lr = 8192 (a power of two: lr * g is exact) and clip_val = 1e-4, so that the bound lr * clip_val = 0.8192 is far above the
    rounding of the update itself: w - lr * g rounds to half an ulp of a weight below 4, 1.2e-7, and the clamp bound
    clip_val * scale to 6e-8 relative - together below the 1e-6 relative margin, which an lr of 1 would not be."""
    import mm2d3d_amd  # noqa: F401

    dev = torch.device("cuda:0")
    lr, val = 8192.0, 1e-4
    tm = _trainer(dev, _nets(dev), lr, precision=precision, gradient_clip_val=val, gradient_clip_algorithm="value")
    w0 = _weights(tm)
    assert float(w0.abs().max()) + lr * val < 4.0
    tm.fit_step(_batch(dev))
    dw = (_weights(tm) - w0).abs()
    at_bound = int((dw >= lr * val * (1 - 1e-6)).sum())
    print(f"precision {precision}: max |dw| {float(dw.max())!r}, bound {lr * val!r}, weights at the bound {at_bound}")
    assert float(dw.max()) <= lr * val * (1 + 1e-6)
    assert at_bound > 0, "no gradient reached the clip value: the bound above was never put to work"
    assert tm.last_grad_norm is None


def test_clipping_is_off_by_default_and_an_unknown_algorithm_raises():
    import mm2d3d_amd  # noqa: F401
    from mm2d3d_amd.train import TrainModel

    mods = {"2d_net": torch.nn.Linear(2, 2), "3d_net": torch.nn.Linear(2, 2)}
    assert TrainModel(mods, None, None, {})._clip is None
    assert TrainModel(mods, None, None, {"gradient_clip_algorithm": "value"})._clip is None  # no value: off, as in Lightning
    assert TrainModel(mods, None, None, {"gradient_clip_val": 0.5})._clip == ("norm", 0.5)
    with pytest.raises(ValueError):
        TrainModel(mods, None, None, {"gradient_clip_val": 0.5, "gradient_clip_algorithm": "l1"})


def test_clipped_step_under_a_forced_one_rank_rccl_reducer_equals_the_step_without_it(monkeypatch):
    """The reducer forced on in a process group of one rank over RCCL, as tests/test_gpu_rccl.py runs it, and that file's
    comparison rule: the parameters are equal bit for bit.  The clip acts on the reduced gradients with the reducer's grad_scale."""
    import torch.distributed as dist

    import mm2d3d_amd  # noqa: F401

    dev = torch.device("cuda:0")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        nets = _nets(dev)
        nets_b = copy.deepcopy(nets[0]), copy.deepcopy(nets[1])
        tk = dict(bn2d_fused=0, bn3d_fused=0, gradient_clip_val=1e-3)  # both on the three-kernel batch norms (what DDP selects)
        monkeypatch.setenv("MM_DDP_FORCE", "1")
        ddp = _trainer(dev, nets, 1.0, **tk)
        monkeypatch.setenv("MM_DDP_FORCE", "0")
        plain = _trainer(dev, nets_b, 1.0, **tk)
        assert ddp.reducer.active and not plain.reducer.active
        for step in range(2):
            la, lb = ddp.fit_step(_batch(dev)), plain.fit_step(_batch(dev))
            torch.cuda.synchronize()
            assert float(la) == float(lb), (step, float(la), float(lb))
            assert float(ddp.last_grad_norm) == float(plain.last_grad_norm) > 1e-3
        assert torch.equal(_weights(ddp), _weights(plain)), "parameters after 2 clipped steps differ"
    finally:
        dist.destroy_process_group()
