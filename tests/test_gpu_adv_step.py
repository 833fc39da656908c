"""Adversarial output alignment in the training step: train_kwargs["lambda_adv"] and ["adv_*"] (mm2d3d_amd/adversarial.py,
losses.adversarial).  Shapes and helpers of tests/_step_util.py: 1 + 1 synthetic nuScenes scenes with 48x64 images, 6 classes, fp16,
dropout p = 0.  The new terms are held to ``losses.adversarial`` evaluated on the logits the heads produced in that very step
(forward hooks) with a copy of the parameters the discriminators had before their step: the same kernels on the same rows, so the
same bits; tests/test_gpu_adv.py holds those kernels to the float64 reference."""
import copy
import socket

import numpy as np
import pytest
import torch

import _adv_ref as R
import _step_util as T
from _step_util import _BUILT, _release_memory, _restore_precision  # noqa: F401  (the autouse fixtures, for this module too)

pytestmark = pytest.mark.gpu

NEW_KEYS = ("train/adv_g_2d", "train/adv_g_3d", "train/adv_d_2d", "train/adv_d_3d", "train/adv_acc_2d", "train/adv_acc_3d")
OLD_KEYS = ("train/loss_segmentation", "train/loss_segmentation_3d", "train/xm_loss_src_2d", "train/xm_loss_tgt_2d", "train/xm_loss_src_3d",
            "train/xm_loss_tgt_3d")
BINDINGS = ("mm_adv_param_count", "mm_adv_ws_bytes", "mm_adv_fwd", "mm_adv_bwd")
MARGIN = 4.43e-8  # of the learning test: 4 x the measured 1.107e-8 (its docstring)


def _trainer(n2, n3, **kw):
    _BUILT.append(T._trainer(n2, n3, **kw))
    return _BUILT[-1]


def _initial(C, H, seed, dev):
    """The two discriminators' parameters as the policy object draws them: one private stream, the 2D head's first."""
    from mm2d3d_amd.adversarial import initial_parameters

    gen = torch.Generator().manual_seed(seed)
    return [initial_parameters(C, H, gen).to(dev) for _ in range(2)]


def _stepped(p0, grad, lr, betas):
    """``p0`` after one step of a separate FlatAdam of the same hyper-parameters on ``grad``."""
    from mm2d3d_amd.optimizers import FlatAdam

    p = torch.nn.Parameter(p0.clone())
    opt = FlatAdam([p], lr=lr, betas=betas)
    opt.grad_arenas()[0].copy_(grad)
    opt.mark_all_touched()
    opt.step()
    return p.detach()


class _CountCalls:
    """Counts the entries into the mm_adv_* bindings of the loaded library."""

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


@pytest.mark.parametrize("joint", [True, False], ids=["joined", "two_calls"])
def test_weight_zero_is_the_step_without_the_options(monkeypatch, joint):
    dev = T._dev()
    n2, n3 = T._nets(dev)
    A = _trainer(copy.deepcopy(n2), copy.deepcopy(n3), joint_domains=joint)
    B = _trainer(n2, n3, joint_domains=joint, lambda_adv=0.0, adv_input="softmax", adv_hidden=16, adv_lr=1e-3, adv_betas=(0.5, 0.9), adv_seed=3)
    calls = _CountCalls(monkeypatch)
    for s in range(2):
        la, lb = A.fit_step(T._batch(dev)), B.fit_step(T._batch(dev))
        assert T._same(la, lb), s
        assert list(A.last_logs) == list(B.last_logs) == list(OLD_KEYS)  # no adv key
        T._assert_same_dicts(A.last_logs, B.last_logs, f"logs of step {s}")
    torch.cuda.synchronize()
    T._assert_same_dicts(A.model.state_dict(), B.model.state_dict(), "weights and running statistics")
    assert A.last_adversary is None and B.last_adversary is None and not B.adversary.built and "adversary" not in B.checkpoint()
    assert calls.n == {name: 0 for name in BINDINGS}
    # the counter counts: the same trainer with the weight raised enters the bindings, once per head and direction
    B.lambda_adv = 0.5
    B.fit_step(T._batch(dev))
    assert calls.n["mm_adv_fwd"] == 2 and calls.n["mm_adv_bwd"] == 2 and B.adversary.built and "train/adv_g_2d" in B.last_logs
    assert "adversary" in B.checkpoint()


@pytest.mark.parametrize("joint", [True, False], ids=["joined", "two_calls"])
@pytest.mark.parametrize("mode", ["selfinfo", "softmax"])
def test_step_adds_the_weighted_terms_and_steps_the_discriminators(mode, joint):
    from mm2d3d_amd.losses import adversarial

    dev = T._dev()
    lam, H, lr, betas, seed = 0.5, 32, 1e-3, (0.9, 0.99), 5
    n2, n3 = T._nets(dev)
    off = _trainer(copy.deepcopy(n2), copy.deepcopy(n3), joint_domains=joint)
    tm = _trainer(n2, n3, joint_domains=joint, lambda_adv=lam, adv_input=mode, adv_hidden=H, adv_lr=lr, adv_betas=betas, adv_seed=seed)
    seen = T._hook_logits(tm)
    batch = T._batch(dev)
    P = int(batch["source"]["x"][0].shape[0])
    loss = tm.fit_step(batch)
    base = off.fit_step(T._batch(dev))
    torch.cuda.synchronize()
    assert list(tm.last_logs) == list(OLD_KEYS) + list(NEW_KEYS) and all(v.is_cuda and v.dim() == 0 for v in tm.last_logs.values())
    for k in OLD_KEYS:  # every other term unchanged in every bit: the discriminators are drawn from a private generator
        assert T._same(tm.last_logs[k], off.last_logs[k]), k
    last = tm.last_adversary
    assert set(last) == {"loss_d", "loss_g", "count", "correct"} and all(v.shape == (2,) and v.is_cuda and not v.requires_grad for v in last.values())
    before = _initial(6, H, seed, dev)
    for i, (net, tag) in enumerate((("2d_net", "2d"), ("3d_net", "3d"))):
        assert len(seen[net]) == (1 if joint else 2)
        x = seen[net][0] if joint else torch.cat(seen[net])
        assert x.shape[1] == 6 and x.shape[0] > P > 0 and (joint or seen[net][0].shape[0] == P)
        want = adversarial(x, P, before[i], mode, H)  # on the step's logits, with the parameters D had before its step
        g, d, acc = (tm.last_logs[f"train/adv_{k}_{tag}"] for k in ("g", "d", "acc"))
        print(f"{mode} {tag}: loss_g {T._f(g):.7g}, loss_d {T._f(d):.7g}, accuracy {T._f(acc):.4f}, count {want['count'].tolist()}, correct {want['correct'].tolist()}")
        assert T._same(g, want["loss_g"]) and T._same(d, want["loss_d"]) and T._f(g) > 0.0 and T._f(d) > 0.0
        assert T._same(acc, want["correct"].sum() / want["count"].sum()) and 0.0 <= T._f(acc) <= 1.0
        assert T._same(last["loss_g"][i], want["loss_g"]) and T._same(last["loss_d"][i], want["loss_d"])
        assert want["count"].tolist() == [P, x.shape[0] - P] and int(last["count"][i]) == x.shape[0] and int(last["correct"][i]) == int(want["correct"].sum())
        # after the step each D is its initial parameters after ONE FlatAdam step on the gradient the kernel reported
        now = tm.adversary.params[i].detach()
        assert T._same(now, _stepped(before[i], want["grad_params"], lr, betas)) and not T._same(now, before[i])
    # the total is the base loss plus lambda times the two terms: both totals carry the float32 roundings of their sums of some
    # ten terms, 1.2e-6 relative each (tests/test_gpu_infomax_step.py), and the two products and sums add as much again
    extra = lam * (T._f(tm.last_logs["train/adv_g_2d"]) + T._f(tm.last_logs["train/adv_g_3d"]))
    print(f"loss {T._f(loss):.7f} = base {T._f(base):.7f} + {extra:.7f}")
    assert extra > 0.0 and abs(T._f(loss) - T._f(base) - extra) <= 4e-6 * max(1.0, abs(T._f(loss)))
    # and the step learnt from them: after one step the weights differ from the twin's without the option
    for name in ("2d_net", "3d_net"):
        a, b = tm.model[name].state_dict(), off.model[name].state_dict()
        assert any(not T._same(a[k], b[k]) for k in a if a[k].is_floating_point() and "running" not in k), name
    assert all(bool(torch.isfinite(v).all()) for v in tm.model.state_dict().values() if v.is_floating_point())
    # D is not one of the trainer's optimisers: the scaler, the clip, the reducer and the EMA never see it
    assert len(tm.optimizers) == 2 and len(tm.checkpoint()["optimizer_states"]) == 2
    assert not any(o is q for o in tm.optimizers for q in tm.adversary.optimizers)


def test_a_skipped_step_leaves_the_networks_and_still_updates_the_discriminators():
    """An inflated initial loss scale: the 16-bit gradients overflow and the device skips the networks' optimiser step.  D's
    gradient comes from the forward's logits, which are valid either way: its step is not gated."""
    dev = T._dev()
    n2, n3 = T._nets(dev)
    tm = _trainer(n2, n3, lambda_adv=0.5, adv_hidden=16, adv_lr=1e-3, loss_scale=dict(init_scale=2.0 ** 40))
    tm.configure_optimizers()
    weights0 = {k: v.detach().clone() for k, v in tm.model.state_dict().items() if v.dtype.is_floating_point and "running" not in k}
    tm.fit_step(T._batch(dev))
    torch.cuda.synchronize()
    assert int(tm.optimizers[0].step_counter().item()) == 0  # skipped on the device
    now = tm.model.state_dict()
    for k, v in weights0.items():
        assert T._same(v, now[k]), k
    before = _initial(6, 16, 0, dev)
    for i in range(2):
        assert not T._same(tm.adversary.params[i].detach(), before[i]) and bool(torch.isfinite(tm.adversary.params[i]).all())
        assert tm.adversary.optimizers[i].step_counter() == 1
    assert all(np.isfinite(T._f(tm.last_logs[k])) for k in NEW_KEYS)


def test_checkpoint_round_trip_resumes_the_discriminators():
    dev = T._dev()
    kw = dict(lambda_adv=0.5, adv_hidden=16, adv_lr=1e-3)
    n2, n3 = T._nets(dev)
    f2, f3 = copy.deepcopy(n2), copy.deepcopy(n3)
    A = _trainer(n2, n3, **kw)
    for _ in range(2):
        A.fit_step(T._batch(dev))
    ck = A.checkpoint()
    sd = ck["adversary"]
    assert (sd["C"], sd["H"], sd["mode"]) == (6, 16, "selfinfo") and len(sd["params"]) == len(sd["optimizers"]) == 2
    assert sd["params"][0].data_ptr() != A.adversary.params[0].data_ptr() and sd["optimizers"][0]["step"] == 2
    B = _trainer(f2, f3, **kw)
    B.load_checkpoint(ck)
    assert B.adversary.built  # from the checkpoint: no step has run in this trainer
    for i in range(2):
        assert T._same(B.adversary.params[i], A.adversary.params[i])
        for name in ("m", "v"):
            assert T._same(B.adversary.optimizers[i]._arenas[0][name], A.adversary.optimizers[i]._arenas[0][name]), name
        assert B.adversary.optimizers[i].step_counter() == 2
    la, lb = A.fit_step(T._batch(dev)), B.fit_step(T._batch(dev))
    torch.cuda.synchronize()
    assert T._same(la, lb)
    T._assert_same_dicts(A.last_logs, B.last_logs, "logs of the step after the resume")
    for i in range(2):
        assert T._same(B.adversary.params[i], A.adversary.params[i])
    # a checkpoint without the key: the discriminators start over from the seed at the next step
    B.load_checkpoint({k: v for k, v in ck.items() if k != "adversary"})
    assert not B.adversary.built
    with pytest.raises(ValueError, match="hidden"):
        _trainer(*T._nets(dev), lambda_adv=0.5, adv_hidden=32).load_checkpoint(ck)


def test_an_active_data_parallel_reducer_is_refused(monkeypatch):
    """The discriminators are stepped per rank and not reduced: under an active reducer ``configure_optimizers`` raises."""
    import torch.distributed as dist

    from mm2d3d_amd import conv2d as _c2d

    dev = T._dev()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    was = _c2d.WGRAD_BATCH[0]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        monkeypatch.setenv("MM_DDP_FORCE", "1")
        tk = dict(bn2d_fused=0, bn3d_fused=0)  # what the reducer selects: nothing for it to switch
        tm = _trainer(*T._nets(dev), lambda_adv=0.5, **tk)
        with pytest.raises(RuntimeError, match="lambda_adv"):
            tm.configure_optimizers()
        assert tm.reducer.active and not tm.adversary.built  # refused before a parameter is broadcast or a discriminator built
    finally:
        dist.destroy_process_group()
        _c2d.WGRAD_BATCH[0] = was


def test_composes_with_coral_and_pseudo_labels():
    dev = T._dev()

    def batch():
        b = T._batch(dev)
        n = int(b["target"]["x"][0].shape[0])
        g = torch.Generator().manual_seed(5)
        for k in ("pseudo_label_2d", "pseudo_label_3d"):
            y = torch.randint(0, 6, (n,), generator=g)
            y[torch.rand(n, generator=g) < 0.5] = -100
            b["target"][k] = y.to(dev)
        return b

    others = dict(lambda_pl=0.5, lambda_coral=0.7)
    n2, n3 = T._nets(dev)
    plain = _trainer(copy.deepcopy(n2), copy.deepcopy(n3), **others)
    both = _trainer(n2, n3, lambda_adv=0.3, adv_hidden=16, **others)
    la, lb = plain.fit_step(batch()), both.fit_step(batch())
    torch.cuda.synchronize()
    assert list(both.last_logs) == list(plain.last_logs) + list(NEW_KEYS) and len(plain.last_logs) > len(OLD_KEYS)
    for k in plain.last_logs:  # the pseudo-label and alignment terms, and every other one, unchanged in every bit
        assert T._same(plain.last_logs[k], both.last_logs[k]), k
    extra = 0.3 * (T._f(both.last_logs["train/adv_g_2d"]) + T._f(both.last_logs["train/adv_g_3d"]))
    assert extra > 0.0 and abs(T._f(lb) - T._f(la) - extra) <= 4e-6 * max(1.0, abs(T._f(lb)))
    assert both.last_coral is not None and both.last_adversary is not None


def test_the_discriminator_learns_to_tell_two_clouds_apart():
    """``losses.adversarial`` + ``FlatAdam`` alone: N = 4096, P = 2048, C = 6, H = 16, two seeded logit clouds (3 * randn, the
    target's scaled by 1.5 and shifted by 2), 100 updates at lr 1e-2; the same loop replayed in float64 on the CPU (tests/_adv_ref.py +
    torch.optim.Adam).  The two trajectories differ by fp32 rounding only.  Measured on an MI355X: loss_D 0.694329 -> 0.643232
    on both sides, the two final values 1.107e-8 apart (relative) - below the fp32 rounding of the output itself; the margin is
    4 x that, 4.43e-8."""
    from mm2d3d_amd.losses import adversarial
    from mm2d3d_amd.optimizers import FlatAdam

    dev = T._dev()
    N, P, C, H, steps, lr, betas = 4096, 2048, 6, 16, 100, 1e-2, (0.9, 0.99)
    x = R.rows(N, C, P, 4242, shift=2.0)
    p0 = R.initial(C, H, seed=11)
    # float64 replay
    th = torch.from_numpy(p0.astype(np.float64)).requires_grad_(True)
    ref_opt = torch.optim.Adam([th], lr=lr, betas=betas)
    ref_losses = []
    for _ in range(steps):
        ref = R.evaluate(x, P, th.detach().numpy(), H, "selfinfo")
        ref_losses.append(ref["loss_d"])
        th.grad = torch.from_numpy(ref["dparams"].copy())
        ref_opt.step()
    ref_final = R.evaluate(x, P, th.detach().numpy(), H, "selfinfo")["loss_d"]
    # the GPU
    xd = torch.from_numpy(x).to(dev)
    p = torch.nn.Parameter(torch.from_numpy(p0).to(dev))
    opt = FlatAdam([p], lr=lr, betas=betas)
    first = None
    for _ in range(steps):
        out = adversarial(xd, P, p.data, "selfinfo", H)
        first = out["loss_d"] if first is None else first
        opt.grad_arenas()[0].copy_(out["grad_params"])
        opt.mark_all_touched()
        opt.step()
    final = adversarial(xd, P, p.data, "selfinfo", H)
    torch.cuda.synchronize()
    first, last = float(first), float(final["loss_d"])
    rel = abs(last - ref_final) / ref_final
    print(f"loss_D {first:.6f} -> {last:.6f} after {steps} updates; float64 replay {ref_losses[0]:.6f} -> {ref_final:.6f}; relative difference {rel:.3e}; "
          f"accuracy {float(final['correct'].sum()) / float(final['count'].sum()):.4f}")
    assert last < first and ref_final < ref_losses[0]
    assert abs(first - ref_losses[0]) <= 1e-5 * max(1.0, ref_losses[0])
    assert rel <= MARGIN

