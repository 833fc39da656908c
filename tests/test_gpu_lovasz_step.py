"""``losses.lovasz_softmax`` under autograd against the C ABI it is made of, and the training step with a registry of
``cross_entropy`` + ``lovasz_softmax`` (the generic branch of mm2d3d_amd/train.py _generic_step) on the small synthetic trainer of
tests/test_gpu_pl_step.py."""
import numpy as np
import pytest
import torch

import test_gpu_pl_step as S

pytestmark = pytest.mark.gpu

LOVASZ = [S.CE[0], {"name": "lovasz_softmax", "weight": 0.5}]
SEG_KEYS = ("train/loss_segmentation", "train/loss_segmentation_3d")


def _abi_gradient(x32, ld, y, grad_out, classes_all=0):
    """(loss, dlogits) of mm_lovasz_fwd + mm_lovasz_bwd on fp32 rows ``ld`` apart."""
    from mm2d3d_amd import _lib

    L = _lib.lib()
    N, C = x32.shape
    err, coef = torch.empty((C, N), device=x32.device), torch.empty((C, N), device=x32.device)
    stats = torch.empty(3, device=x32.device)
    ws = torch.empty(int(L.mm_lovasz_ws_bytes(N, C)), dtype=torch.uint8, device=x32.device)
    _lib.check(L.mm_lovasz_fwd(x32.data_ptr(), ld, N, C, y.data_ptr(), -100, classes_all, err.data_ptr(), coef.data_ptr(), stats.data_ptr(),
                               ws.data_ptr(), ws.numel(), _lib.stream()), "lovasz_fwd")
    g = torch.tensor([grad_out], dtype=torch.float32, device=x32.device)
    d = torch.empty((N, C), device=x32.device)
    _lib.check(L.mm_lovasz_bwd(x32.data_ptr(), ld, N, C, coef.data_ptr(), g.data_ptr(), d.data_ptr(), C, _lib.stream()), "lovasz_bwd")
    return stats[0], d


@pytest.mark.parametrize("kind", ["fp32", "fp16", "row_slice", "scaled", "all"])
def test_autograd_gives_the_bits_of_the_backward_kernel_on_the_forwards_own_coefficients(kind):
    from mm2d3d_amd.losses import lovasz_softmax

    dev = S._dev()
    g = torch.Generator().manual_seed(3)
    N, P, C = 2500, 1300, 6
    full = (3 * torch.randn(N, C, generator=g)).to(dev)
    y = torch.randint(0, C, (N,), generator=g)
    y[torch.rand(N, generator=g) < 0.2] = -100
    y = y.to(dev)
    if kind == "fp16":
        full = full.half()
    full.requires_grad_(True)
    rows = P if kind == "row_slice" else N
    scale = 1024.0 if kind == "scaled" else 1.0
    loss = lovasz_softmax(full[:rows] if kind == "row_slice" else full, y[:rows], classes="all" if kind == "all" else "present")
    (loss * scale).backward()
    x32 = full.detach().float()
    ref_loss, d = _abi_gradient(x32[:rows], C, y[:rows].contiguous(), scale, 1 if kind == "all" else 0)
    assert loss.item() == ref_loss.item() and 0.0 < loss.item() < 1.0
    assert full.grad.dtype == full.dtype and full.grad.shape == full.shape
    assert torch.equal(full.grad[:rows], d.to(full.dtype)) and d.abs().max().item() > 0
    assert not full.grad[rows:].any()
    assert not full.grad[:rows][y[:rows] == -100].any()


def _trainer(dev, cfg, **kw):
    from mm2d3d_amd.losses import Loss
    from mm2d3d_amd.optimizers import Optimizer
    from mm2d3d_amd.train import TrainModel

    n2, n3 = S._nets(dev)
    return TrainModel({"2d_net": n2, "3d_net": n3}, {"2d_net": Optimizer("adamw", lr=1e-3), "3d_net": Optimizer("adamw", lr=1e-3)}, Loss(cfg),
                      dict(lambda_xm_src=1.0, lambda_xm_trg=0.1, gc_freeze=False, num_classes=6, **kw))


def _two_steps(dev, cfg, **kw):
    """(logs of the first step, parameters after it, total of the second step) of a fresh trainer on the seeded nets and batches."""
    tm = _trainer(dev, cfg, **kw)
    pseudo = kw.get("lambda_pl", 0.0) > 0
    tm.fit_step(S._batch(dev, pseudo=pseudo))
    logs = {k: v.item() for k, v in tm.last_logs.items()}
    params = [p.detach().clone() for p in tm.model.parameters()]
    second = tm.fit_step(S._batch(dev, pseudo=pseudo)).item()
    tm.drain()
    torch.cuda.synchronize()
    return tm, logs, params, second


@pytest.mark.parametrize("kw", [dict(), dict(lambda_pl=0.5, pseudo_label_source="batch")], ids=["plain", "pseudo_labels"])
def test_two_fit_steps_with_cross_entropy_plus_lovasz(kw):
    dev = S._dev()
    ce_tm, ce, ce_params, ce_second = _two_steps(dev, S.CE, **kw)
    lv_tm, lv, lv_params, lv_second = _two_steps(dev, LOVASZ, **kw)
    assert ce_tm._single_cross_entropy() is not None and lv_tm._single_cross_entropy() is None
    assert str(lv_tm.loss) == "cross_entropy[weight=" + str(S.W) + "]+0.5lovasz_softmax"
    assert set(lv) == set(ce) and (len(lv) == 8 if kw else len(lv) == 6)
    for k in SEG_KEYS:
        # the same weights and batch: the same logits, and 0.5 * a Lovasz term in (0, 1] on top of the cross entropy
        print(k, lv[k], ce[k])
        assert np.isfinite(lv[k]) and ce[k] < lv[k] <= ce[k] + 0.5 * (1 + 1e-6), k
    for k in lv:
        if k not in SEG_KEYS:
            assert abs(lv[k] - ce[k]) <= 1e-6 * max(1.0, abs(ce[k])), k  # the other terms see the same logits
    assert any(not torch.equal(a, b) for a, b in zip(lv_params, ce_params))
    assert np.isfinite(lv_second) and np.isfinite(ce_second)


def test_a_lovasz_entry_of_weight_zero_leaves_the_cross_entropy_bits_alone():
    """Without pseudo labels both registries go through ``self.loss("segmentation", ...)``: ce + 0.0 * lovasz is ce, bit for bit, and a
    registry of one cross_entropy entry is still what _single_cross_entropy recognises."""
    dev = S._dev()
    ce_tm, ce, _, _ = _two_steps(dev, S.CE)
    again_tm, again, _, _ = _two_steps(dev, S.CE)
    zero_tm, zero, _, _ = _two_steps(dev, [S.CE[0], {"name": "lovasz_softmax", "weight": 0.0}])
    assert ce_tm._single_cross_entropy() == (1.0, S.W) and zero_tm._single_cross_entropy() is None
    assert ce == again
    for k in SEG_KEYS:
        assert zero[k] == ce[k], k
