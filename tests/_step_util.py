"""Helpers shared by the step tests tests/test_gpu_teacher_step.py, test_gpu_soft_step.py and test_gpu_adaptive_step.py (no tests
here): 1 + 1 synthetic nuScenes scenes with 48x64 images, 6 classes, fp16, dropout p = 0, ema_decay 0.9.  A test module that uses
them imports the autouse fixture ``_restore_precision`` too; ``_release_memory`` is for modules that build through ``_BUILT``."""
import pytest
import torch

W = [1.9241476, 1.0, 2.16763851, 2.78254323, 1.54875664, 1.85686537]
NET3D = dict(in_channels=3, m=16, full_scale=4096, num_planes=7)
CE = [{"name": "cross_entropy", "target": "segmentation", "args": {"weight": W}}]
DECAY = 0.9


def _dev():
    import mm2d3d_amd  # noqa: F401

    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_precision():
    from mm2d3d_amd import nn2d, scn

    try:
        yield
    finally:
        nn2d.set_precision(nn2d.DEFAULT_PRECISION)
        scn.set_activation_dtype(torch.float32)


def _nets(dev, seed=0, head_scale=1.0, head_scale_2d=None):
    from mm2d3d_amd.net2d import Net2DSeg
    from mm2d3d_amd.net3d import Net3DSeg

    torch.manual_seed(seed)
    n2, n3 = Net2DSeg(6, pretrained=False), Net3DSeg(6, True, NET3D)
    for m in n2.modules():  # dropout is random: off, for parity between the sides
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    if head_scale != 1.0:  # larger logits: wider gaps between the two best classes, and confidences on both sides of a threshold
        with torch.no_grad():
            n2.con1_1_avg.weight.mul_(head_scale if head_scale_2d is None else head_scale_2d), n3.linear.weight.mul_(head_scale)
    return n2.to(dev), n3.to(dev)


def _batch(dev):
    from mm2d3d_amd.synthetic import make_batch

    return {"source": make_batch(5, 1, "nuscenes", (48, 64), device=dev), "target": make_batch(6, 1, "nuscenes", (48, 64), device=dev)}


def _trainer(n2, n3, lr=1e-3, **kw):
    from mm2d3d_amd.losses import Loss
    from mm2d3d_amd.optimizers import Optimizer
    from mm2d3d_amd.train import TrainModel

    return TrainModel({"2d_net": n2, "3d_net": n3}, {k: Optimizer("adamw", lr=lr) for k in ("2d_net", "3d_net")}, Loss(CE),
                      dict(lambda_xm_src=1.0, lambda_xm_trg=0.1, gc_freeze=False, precision="fp16", ema_decay=DECAY, **kw))


def _bits(t):
    t = t.detach().contiguous().reshape(-1)
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _f(t):
    return float(t.detach())


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _assert_same_dicts(a, b, what):
    assert list(a) == list(b), what
    for k in a:
        assert _same(a[k], b[k]), (what, k)


def _alone_logits(tm, dev):
    """The teacher's logits of the target batch ALONE: an eval forward under ``ema.applied()``, outside any step."""
    trg = _batch(dev)["target"]
    with torch.no_grad(), tm._use(), tm.ema.applied():
        tm.model.eval()
        l2 = tm(trg, model_name="2d_net")[0]["seg_logit"].clone()
        l3 = tm(trg, model_name="3d_net")[0]["seg_logit"].clone()
    tm.model.train()
    return l2, l3


def _hook_logits(tm, keep=lambda t: t.detach().clone()):
    """The main heads' logits of every forward of the two networks, in call order, kept on the device as they were (or as ``keep``
    makes them)."""
    seen = {"2d_net": [], "3d_net": []}
    for name in seen:
        tm.model[name].register_forward_hook(lambda m, i, out, name=name: seen[name].append(keep(out[0]["seg_logit"])))
    return seen


_BUILT = []  # the trainers of the running test


def _dispose(tm):
    """Lets a finished trainer's device memory go.  A flat optimiser's post-accumulate hooks close over its arena, whose ``params``
    list holds the parameters the hooks hang on: a cycle through the tensors that the collector does not take apart, so a trainer
    that is merely dropped keeps about 1 GiB of arenas for the life of the process (measured: 1.02 GiB per trainer dropped, 0.08
    after this).  Emptying the arenas and the hook tables breaks it."""
    for opt in tm.optimizers:
        for a in opt._arenas:
            if a is not None:
                a.clear()
    for q in tm.model.parameters():
        hooks = getattr(q, "_post_accumulate_grad_hooks", None)
        if hooks is not None:
            hooks.clear()
        q.__dict__.pop("_mm_hooks", None)


@pytest.fixture(autouse=True)
def _release_memory():
    """The suite runs in one process, which the step tests of the other files fill close to the device's capacity, so this file
    hands back what it takes.  Its 2D trunks run eagerly (graph2d.ENABLED off for the test: the same kernels, launched one by
    one) - a captured graph keeps a private memory pool - and every trainer a test built is taken apart once the test is over."""
    import gc

    from mm2d3d_amd import graph2d

    was = graph2d.ENABLED[0]
    graph2d.ENABLED[0] = False
    try:
        yield
    finally:
        graph2d.ENABLED[0] = was
        for tm in _BUILT:
            _dispose(tm)
        del _BUILT[:]
        gc.collect()
        torch.cuda.empty_cache()
