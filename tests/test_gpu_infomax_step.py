"""Target-domain entropy and diversity in the training step: train_kwargs["lambda_minent"], ["lambda_div"] and ["div_prior"]
(mm2d3d_amd/infomax.py, losses.target_entropy).  Shapes and helpers of tests/_step_util.py: 1 + 1 synthetic nuScenes scenes with
48x64 images, 6 classes, fp16, dropout p = 0.  The four new terms are held to the float64 reference tests/_infomax_ref.py, evaluated
on the logits the heads produced in that very step (forward hooks), at the loss tolerance of tests/test_gpu_infomax.py."""
import copy

import numpy as np
import pytest
import torch

import _infomax_ref as R
import _step_util as T
from _step_util import _BUILT, _release_memory, _restore_precision  # noqa: F401  (the autouse fixtures, for this module too)

pytestmark = pytest.mark.gpu

NEW_KEYS = ("train/minent_tgt_2d", "train/minent_tgt_3d", "train/div_tgt_2d", "train/div_tgt_3d")
OLD_KEYS = ("train/loss_segmentation", "train/loss_segmentation_3d", "train/xm_loss_src_2d", "train/xm_loss_tgt_2d", "train/xm_loss_src_3d",
            "train/xm_loss_tgt_3d")
PRIOR = [3.0, 1.0, 2.0, 1.0, 0.5, 2.5]
ON = dict(lambda_minent=0.3, lambda_div=0.2)


def _trainer(n2, n3, **kw):
    _BUILT.append(T._trainer(n2, n3, **kw))
    return _BUILT[-1]


def _close(got, ref):
    return abs(got - ref) <= 1e-5 * max(1.0, abs(ref))


def _hook_logits(tm):
    """The main heads' logits of every forward of the two networks, in call order, as float32 arrays on the host."""
    return T._hook_logits(tm, lambda t: t.detach().float().cpu().numpy())


def test_both_weights_zero_is_the_step_without_the_options():
    dev = T._dev()
    n2, n3 = T._nets(dev)
    A = _trainer(copy.deepcopy(n2), copy.deepcopy(n3))
    B = _trainer(n2, n3, lambda_minent=0.0, lambda_div=0.0, div_prior=PRIOR)
    for s in range(2):
        la, lb = A.fit_step(T._batch(dev)), B.fit_step(T._batch(dev))
        assert T._same(la, lb), s
        assert list(A.last_logs) == list(B.last_logs) == list(OLD_KEYS)  # no new log key
        T._assert_same_dicts(A.last_logs, B.last_logs, f"logs of step {s}")
    torch.cuda.synchronize()
    T._assert_same_dicts(A.model.state_dict(), B.model.state_dict(), "weights and running statistics")
    T._assert_same_dicts(A.ema.teacher_state_dict(), B.ema.teacher_state_dict(), "teacher")
    assert B.last_target_mass is None and A.last_target_mass is None


@pytest.mark.parametrize("prior", [None, PRIOR], ids=["uniform", "prior"])
def test_joined_step_adds_the_weighted_terms(prior):
    dev = T._dev()
    n2, n3 = T._nets(dev)
    off = _trainer(copy.deepcopy(n2), copy.deepcopy(n3))
    tm = _trainer(n2, n3, div_prior=prior, **ON)
    seen = _hook_logits(tm)
    batch = T._batch(dev)
    P = int(batch["source"]["x"][0].shape[0])
    loss = tm.fit_step(batch)
    off.fit_step(T._batch(dev))
    torch.cuda.synchronize()
    logs = {k: T._f(v) for k, v in tm.last_logs.items()}
    assert list(logs) == list(OLD_KEYS) + list(NEW_KEYS) and all(v.is_cuda and v.dim() == 0 for v in tm.last_logs.values())
    # the returned loss is the weighted sum of the ten logged terms, which are all >= 0: ten float32 products and ten sums, each
    # rounding <= 2^-24 of a partial sum that the total bounds: 20 * 2^-24 = 1.2e-6 relative
    lam = {"segmentation": 1.0, "xm_loss_src": 1.0, "xm_loss_tgt": 0.1, "minent": 0.3, "div": 0.2}
    want = sum(next(w for n, w in lam.items() if n in k) * np.float64(v) for k, v in logs.items())
    print(f"loss {T._f(loss):.7f}, weighted sum of the logged terms {want:.7f}")
    assert abs(T._f(loss) - want) <= 2e-6 * max(1.0, abs(want))
    # the four terms against the reference on this step's logits: one joined forward per network, rows [P, N) the target's
    assert len(seen["2d_net"]) == 1 and len(seen["3d_net"]) == 1
    mass = tm.last_target_mass
    assert mass.shape == (2, 6) and mass.dtype == torch.float32 and mass.is_cuda and not mass.requires_grad
    for o, (net, tag) in enumerate((("2d_net", "2d"), ("3d_net", "3d"))):
        x = seen[net][0]
        assert x.shape[1] == 6 and x.shape[0] > P > 0
        ref = R.forward(x, P, prior)
        ent, div = logs[f"train/minent_tgt_{tag}"], logs[f"train/div_tgt_{tag}"]
        print(f"{tag}: ent {ent:.7f} ref {ref['ent']:.7f}  div {div:.7f} ref {ref['div']:.7f}  count {ref['count']} of {x.shape[0] - P}")
        assert ref["count"] == x.shape[0] - P and _close(ent, ref["ent"]) and _close(div, ref["div"])
        assert 0.0 < ent <= 1.0 and div >= 0.0
        assert abs(float(mass[o].sum()) - 1.0) <= 1e-5
        assert np.abs(mass[o].cpu().double().numpy() - ref["mass"]).max() <= 1e-5
    # and the step learnt from them: after one step the weights differ from the twin's without the options
    for name in ("2d_net", "3d_net"):
        a, b = tm.model[name].state_dict(), off.model[name].state_dict()
        assert any(not T._same(a[k], b[k]) for k in a if a[k].is_floating_point() and "running" not in k), name
    assert all(bool(torch.isfinite(v).all()) for v in tm.model.state_dict().values() if v.is_floating_point())


def test_joined_pass_equals_the_two_call_sequence():
    """Tolerances of tests/test_gpu_pl_step.py::test_joined_pass_equals_the_two_call_sequence: 2e-3 * max(1, |v|) for terms that
    pass through the 16-bit 2D branch; in the two-call path the terms are taken on the target pass's logits with first_row 0."""
    dev = T._dev()
    n2, n3 = T._nets(dev)
    two = _trainer(copy.deepcopy(n2), copy.deepcopy(n3), joint_domains=False, div_prior=PRIOR, **ON)
    one = _trainer(n2, n3, div_prior=PRIOR, **ON)
    seen = _hook_logits(two)
    two.training_step(T._batch(dev)).backward()
    one.training_step(T._batch(dev)).backward()
    torch.cuda.synchronize()
    assert list(one.last_logs) == list(two.last_logs) == list(OLD_KEYS) + list(NEW_KEYS)
    for k in NEW_KEYS:
        a, b = T._f(one.last_logs[k]), T._f(two.last_logs[k])
        print(f"{k}: joined {a:.7f} two calls {b:.7f}")
        assert abs(a - b) < 2e-3 * max(1.0, abs(b)), k
    # the two-call path's own terms: the SECOND forward of each network is the target pass, every row a target row
    for net, tag in (("2d_net", "2d"), ("3d_net", "3d")):
        assert len(seen[net]) == 2
        ref = R.forward(seen[net][1], 0, PRIOR)
        assert _close(T._f(two.last_logs[f"train/minent_tgt_{tag}"]), ref["ent"]) and _close(T._f(two.last_logs[f"train/div_tgt_{tag}"]), ref["div"])
    assert torch.allclose(one.last_target_mass, two.last_target_mass, atol=2e-3, rtol=0)


@pytest.mark.parametrize("joint", [True, False], ids=["joined", "two_calls"])
def test_composes_with_the_pseudo_label_loss(joint):
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

    n2, n3 = T._nets(dev)
    plain = _trainer(copy.deepcopy(n2), copy.deepcopy(n3), lambda_pl=0.5, joint_domains=joint)
    both = _trainer(n2, n3, lambda_pl=0.5, joint_domains=joint, **ON)
    la, lb = plain.fit_step(batch()), both.fit_step(batch())
    torch.cuda.synchronize()
    assert set(both.last_logs) == set(plain.last_logs) | set(NEW_KEYS) and len(plain.last_logs) == 8
    for k in plain.last_logs:  # the pseudo-label terms, and every other one, unchanged in every bit
        assert T._same(plain.last_logs[k], both.last_logs[k]), k
    extra = sum(w * T._f(both.last_logs[k]) for k, w in zip(NEW_KEYS, (0.3, 0.3, 0.2, 0.2)))
    # both totals carry the float32 roundings of their sums (1.2e-6 relative each, as above)
    assert extra > 0.0 and abs(T._f(lb) - T._f(la) - extra) <= 4e-6 * max(1.0, abs(T._f(lb)))


def test_a_prior_of_the_wrong_length_is_refused_before_the_step_launches_anything():
    dev = T._dev()
    tm = _trainer(*T._nets(dev), lambda_div=0.2, div_prior=[1.0, 2.0, 3.0, 4.0, 5.0])
    tm.configure_optimizers()
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in tm.model.state_dict().items()}
    with pytest.raises(ValueError, match=r"div_prior.*5 entries.*C = 6"):
        tm.fit_step(T._batch(dev))
    torch.cuda.synchronize()
    # no forward ran: not one running statistic or batch counter moved, nothing was logged
    T._assert_same_dicts(before, tm.model.state_dict(), "state after the refusal")
    assert tm.global_step == 0 and tm.last_logs == {} and tm.last_target_mass is None
    # the right length trains
    ok = _trainer(*T._nets(dev), lambda_div=0.2, div_prior=PRIOR)
    assert np.isfinite(T._f(ok.fit_step(T._batch(dev))))
