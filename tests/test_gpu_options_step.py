"""Every optional term of the training step at once (train.OPTIONS: pseudo labels, MinEnt / InfoMax, CORAL, the output adversary, FDA
and the dense cross-modal window), in the joined and in the two-call pass.  Shapes and helpers of tests/_step_util.py: 1 + 1
synthetic nuScenes scenes with 48x64 images, 6 classes, fp16, dropout p = 0.  What is held here is what the step's shared tail
promises: the order of the logged keys, and a loss that is the logged terms under the same float32 operations in the same order,
so the same bits.  Each term's own value is held by the option's own step test."""
import pytest
import torch

import _step_util as T
from _step_util import _BUILT, _release_memory, _restore_precision  # noqa: F401  (the autouse fixtures, for this module too)
from test_gpu_xmdense import _room_on_the_device  # noqa: F401  (module-scoped, autouse: once more before this module's first test)

pytestmark = pytest.mark.gpu

ON = dict(lambda_pl=0.5, lambda_minent=0.3, lambda_div=0.2, lambda_coral=0.5, lambda_adv=0.1, fda_beta=0.05, xm_window=2)
KEYS = ["loss_segmentation", "loss_segmentation_3d", "xm_loss_src_2d", "xm_loss_tgt_2d", "xm_loss_src_3d", "xm_loss_tgt_3d",  # the six base keys
        "xm_moved_2d", "xm_shift_2d", "xm_moved_3d", "xm_shift_3d",  # the dense window
        "pl_loss_tgt_2d", "pl_loss_tgt_3d",  # pseudo labels of the batch
        "minent_tgt_2d", "minent_tgt_3d", "div_tgt_2d", "div_tgt_3d",  # MinEnt / InfoMax
        "coral_2d", "coral_3d",
        "adv_g_2d", "adv_g_3d", "adv_d_2d", "adv_d_3d", "adv_acc_2d", "adv_acc_3d",
        "fda_mse"]


def _batch(dev):
    b = T._batch(dev)
    n = int(b["target"]["x"][0].shape[0])
    g = torch.Generator().manual_seed(5)
    for k in ("pseudo_label_2d", "pseudo_label_3d"):
        y = torch.randint(0, 6, (n,), generator=g)
        y[torch.rand(n, generator=g) < 0.5] = -100
        b["target"][k] = y.to(dev)
    return b


def _loss_from_logs(tm):
    """The step's loss from its logged terms: the float32 operations of the step's tail, in its order."""
    v = {k.split("/", 1)[1]: t.detach() for k, t in tm.last_logs.items()}
    branches = []
    for d in ("2d", "3d"):
        seg = v["loss_segmentation" if d == "2d" else "loss_segmentation_3d"]
        loss = seg + tm.lambda_xm_src * v[f"xm_loss_src_{d}"] + tm.lambda_xm_trg * v[f"xm_loss_tgt_{d}"]
        loss = loss + tm.lambda_pl * v[f"pl_loss_tgt_{d}"]
        loss = loss + tm.lambda_minent * v[f"minent_tgt_{d}"] + tm.lambda_div * v[f"div_tgt_{d}"]
        loss = loss + tm.lambda_coral * v[f"coral_{d}"]
        loss = loss + tm.lambda_adv * v[f"adv_g_{d}"]
        branches.append(loss)
    return branches[0] + branches[1]


@pytest.mark.parametrize("joint", [True, False], ids=["joined", "two_calls"])
def test_all_options_together_log_in_order_and_sum_to_the_loss(joint):
    dev = T._dev()
    _BUILT.append(T._trainer(*T._nets(dev, head_scale=8.0), joint_domains=joint, **ON))
    tm = _BUILT[-1]
    assert all(o.active for o in tm._options if o is not tm.selftrain) and tm.lambda_pl > 0
    for step in range(2):
        loss = tm.fit_step(_batch(dev))
        torch.cuda.synchronize()
        assert list(tm.last_logs) == [f"train/{k}" for k in KEYS], step
        assert all(t.is_cuda and t.dim() == 0 and t.dtype == torch.float32 for t in tm.last_logs.values())
        want = _loss_from_logs(tm)
        print(f"step {step}: loss {T._f(loss):.7f}, from the logged terms {T._f(want):.7f}")
        assert T._f(loss) == T._f(loss) and want.dtype == loss.dtype == torch.float32
        assert T._same(loss, want), (step, T._f(loss), T._f(want))
    # every option left its state behind, and the optional checkpoint entry is the adversary's alone (no adaptive thresholds here)
    assert all(getattr(tm, k) is not None for k in ("last_target_mass", "last_coral", "last_adversary", "last_fda", "last_match"))
    ckpt = tm.checkpoint()
    assert "adversary" in ckpt and "pl_adaptive" not in ckpt
