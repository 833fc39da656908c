"""Fourier domain adaptation in the training step: train_kwargs["fda_beta"] and ["fda_image_norm"] (mm2d3d_amd/fda.py).  Shapes and
helpers of tests/_step_util.py: 1 + 1 synthetic nuScenes scenes with 48x64 images, 6 classes, fp16, dropout p = 0.  The images the
2D network receives (a forward pre-hook) are held to ``fda_transfer`` on the batch's own images: the same kernels on the same pixels,
so the same bits; tests/test_gpu_fda.py holds those kernels to the float64 reference."""
import copy

import pytest
import torch

import _step_util as T
from _step_util import _BUILT, _release_memory, _restore_precision  # noqa: F401  (the autouse fixtures, for this module too)

pytestmark = pytest.mark.gpu

OLD_KEYS = ("train/loss_segmentation", "train/loss_segmentation_3d", "train/xm_loss_src_2d", "train/xm_loss_tgt_2d", "train/xm_loss_src_3d",
            "train/xm_loss_tgt_3d")
BETA = 0.09  # a band of floor(48 * 0.09) = 4
BINDINGS = ("mm_fda_ws_bytes", "mm_fda_transfer")


def _trainer(n2, n3, **kw):
    _BUILT.append(T._trainer(n2, n3, **kw))
    return _BUILT[-1]


def _hook_images(tm):
    """The images of every forward of the 2D network, in call order, kept on the device as they were."""
    seen = []
    tm.model["2d_net"].register_forward_pre_hook(lambda m, args: seen.append(args[0]["img"].detach().clone()))
    return seen


class _CountCalls:
    """Counts the entries into the mm_fda_* bindings of the loaded library."""

    def __init__(self, monkeypatch):
        from mm2d3d_amd import _lib

        L = _lib.lib()
        self.n = {}
        for name in BINDINGS:
            self.n[name] = 0
            monkeypatch.setattr(L, name, self._wrap(name, getattr(L, name)))

    def _wrap(self, name, fn):
        def call(*a):
            self.n[name] += 1
            return fn(*a)

        return call


def _snapshot(batch):
    """The tensors a step must leave alone, as objects and as contents."""
    keep = {}
    for dom in ("source", "target"):
        b = batch[dom]
        keep[dom] = dict(keys=list(b), img=b["img"], depth=b["depth"], x0=b["x"][0], indices=b["img_indices"],
                         img_bits=b["img"].clone(), depth_bits=b["depth"].clone(), x0_bits=b["x"][0].clone(),
                         index_bits=[torch.as_tensor(i).clone() for i in b["img_indices"]])
    return keep


def _assert_untouched(batch, keep):
    for dom in ("source", "target"):
        b, k = batch[dom], keep[dom]
        assert [key for key in b if not key.startswith("_")] == k["keys"], dom  # (the networks cache their "_..." entries in a batch)
        # (x[1] is not held to this: in the two-call path the 3D network gates it in place, with or without the option)
        assert b["img"] is k["img"] and b["depth"] is k["depth"] and b["x"][0] is k["x0"], dom
        assert b["img_indices"] is k["indices"], dom
        assert T._same(b["img"], k["img_bits"]) and T._same(b["depth"], k["depth_bits"]) and torch.equal(b["x"][0], k["x0_bits"]), dom
        assert all(torch.equal(torch.as_tensor(i), j) for i, j in zip(b["img_indices"], k["index_bits"])), dom


def test_beta_none_is_the_step_without_the_option(monkeypatch):
    dev = T._dev()
    n2, n3 = T._nets(dev)
    A = _trainer(copy.deepcopy(n2), copy.deepcopy(n3))
    B = _trainer(n2, n3, fda_beta=None, fda_image_norm=([0.5] * 3, [0.25] * 3))
    calls = _CountCalls(monkeypatch)
    for s in range(2):
        la, lb = A.fit_step(T._batch(dev)), B.fit_step(T._batch(dev))
        assert T._same(la, lb), s
        assert list(A.last_logs) == list(B.last_logs) == list(OLD_KEYS)  # no new key
        T._assert_same_dicts(A.last_logs, B.last_logs, f"logs of step {s}")
    torch.cuda.synchronize()
    T._assert_same_dicts(A.model.state_dict(), B.model.state_dict(), "weights and running statistics")
    assert A.last_fda is None and B.last_fda is None
    assert calls.n == {k: 0 for k in BINDINGS}
    # the counter counts: the same trainer with the option set enters the bindings once per step
    B.fda_beta = BETA
    B.fit_step(T._batch(dev))
    assert calls.n == {k: 1 for k in BINDINGS} and "train/fda_mse" in B.last_logs


@pytest.mark.parametrize("joint", [True, False], ids=["joined", "two_calls"])
def test_the_2d_network_receives_the_styled_source_images(joint, monkeypatch):
    from mm2d3d_amd.fda import fda_transfer

    dev = T._dev()
    n2, n3 = T._nets(dev)
    tm = _trainer(n2, n3, joint_domains=joint, fda_beta=BETA)
    seen = _hook_images(tm)
    batch, nxt = T._batch(dev), T._batch(dev)
    nxt["source"]["img"] = nxt["source"]["img"].flip(-1).contiguous()  # another batch, so that a stale image would show
    for step, (cur, following) in enumerate(((batch, nxt), (nxt, None))):  # the second step's batch was joined one step ahead
        keep = _snapshot(cur)
        want = fda_transfer(cur["source"]["img"], cur["target"]["img"], BETA)
        del seen[:]
        loss = tm.fit_step(cur, next_batch=following)
        torch.cuda.synchronize()
        B = int(cur["source"]["img"].shape[0])
        got_src, got_trg = (seen[0][:B], seen[0][B:]) if joint else (seen[0], seen[1])
        assert len(seen) == (1 if joint else 2), step
        assert T._same(got_src, want["img"]), step  # fda_transfer's bits on the source rows
        assert T._same(got_trg, cur["target"]["img"]), step  # the batch's own bits on the target rows
        assert not T._same(want["img"], cur["source"]["img"])
        _assert_untouched(cur, keep)
        last = tm.last_fda
        assert set(last) == {"img", "band", "mse"} and last["band"] == want["band"] == 4
        assert T._same(last["img"], want["img"]) and T._same(last["mse"], want["mse"]) and last["mse"].is_cuda
        assert list(tm.last_logs) == list(OLD_KEYS) + ["train/fda_mse"]
        mse = tm.last_logs["train/fda_mse"]
        assert mse.is_cuda and mse.dim() == 0 and T._same(mse, want["mse"].mean()) and T._f(mse) > 0.0
        assert torch.isfinite(loss).item()
    # validation never styles anything
    calls = _CountCalls(monkeypatch)
    del seen[:]
    val = T._batch(dev)["target"]
    tm.validation_step(val)
    torch.cuda.synchronize()
    assert calls.n == {k: 0 for k in BINDINGS} and len(seen) == 1 and T._same(seen[0], val["img"])
    tm.model.train()


def test_image_norm_reaches_the_kernel():
    from mm2d3d_amd.fda import fda_transfer

    dev = T._dev()
    norm = ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
    n2, n3 = T._nets(dev)
    tm = _trainer(n2, n3, fda_beta=BETA, fda_image_norm=norm)
    seen = _hook_images(tm)
    batch = T._batch(dev)
    # normalised source images of a negative mean: the pixels' DC term is positive, the tensor's is not - only where the two differ
    # in sign does the normaliser change the result
    batch["source"]["img"] = batch["source"]["img"] - 0.8
    tm.fit_step(batch)
    want = fda_transfer(batch["source"]["img"], batch["target"]["img"], BETA, norm)
    plain = fda_transfer(batch["source"]["img"], batch["target"]["img"], BETA)
    assert T._same(seen[0][:1], want["img"]) and not T._same(want["img"], plain["img"])


def test_source_and_target_images_of_different_sizes_raise():
    from mm2d3d_amd.synthetic import make_batch

    dev = T._dev()
    n2, n3 = T._nets(dev)
    tm = _trainer(n2, n3, fda_beta=BETA)
    batch = {"source": make_batch(5, 1, "nuscenes", (48, 64), device=dev), "target": make_batch(6, 1, "nuscenes", (40, 64), device=dev)}
    with pytest.raises(ValueError, match="must agree in C, H and W"):
        tm.fit_step(batch)
