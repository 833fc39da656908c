"""The self-training step: train_kwargs["lambda_pl"] adds the pseudo-label cross entropy of the target rows to both branches
(mm2d3d_amd/train.py, losses.cross_entropy_pair) - against the CPU oracle, across both step paths, label modes and registries."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _pselab_util import KW, write_scenes

pytestmark = pytest.mark.gpu

W = [1.9241476, 1.0, 2.16763851, 2.78254323, 1.54875664, 1.85686537]
NET3D = dict(in_channels=3, m=16, full_scale=4096, num_planes=7)
CE = [{"name": "cross_entropy", "target": "segmentation", "args": {"weight": W}}]
PL_KEYS = ("train/pl_loss_tgt_2d", "train/pl_loss_tgt_3d")


def _dev():
    import mm2d3d_amd  # noqa: F401

    return torch.device("cuda:0")


def _nets(dev=None, seed=0):
    from mm2d3d_amd.net2d import Net2DSeg
    from mm2d3d_amd.net3d import Net3DSeg

    torch.manual_seed(seed)
    n2, n3 = Net2DSeg(6, pretrained=False), Net3DSeg(6, True, NET3D)
    for m in n2.modules():  # dropout is random: off, for parity between the sides
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return (n2, n3) if dev is None else (n2.to(dev), n3.to(dev))


def _pseudo(n, seed):
    """Seeded pseudo labels of a target batch: about half are -100; the three arrays differ."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k in ("pseudo_label_2d", "pseudo_label_3d", "pseudo_label_ensemble"):
        y = torch.randint(0, 6, (n,), generator=g)
        y[torch.rand(n, generator=g) < 0.5] = -100
        out[k] = y
    return out


def _batch(dev, n_src=1, pseudo=True, **swap):
    """1 (or 2) + 1 scenes with 48x64 images; ``swap``: batch key -> the key whose array it gets instead."""
    from mm2d3d_amd.synthetic import make_batch

    b = {"source": make_batch(5, n_src, "nuscenes", (48, 64), device=dev), "target": make_batch(6, 1, "nuscenes", (48, 64), device=dev)}
    if pseudo:
        ps = _pseudo(int(b["target"]["x"][0].shape[0]), 77)
        for k in ps:
            v = ps[swap.get(k, k)]
            b["target"][k] = v if dev is None else v.to(dev)
    return b


def _trainer(n2, n3, cfg=CE, **kw):
    from mm2d3d_amd.losses import Loss
    from mm2d3d_amd.train import TrainModel

    return TrainModel({"2d_net": n2, "3d_net": n3}, None, Loss(cfg), dict(lambda_xm_src=1.0, lambda_xm_trg=0.1, gc_freeze=False, **kw))


def _oracle_step(sd2d, net3d, batch, lambda_pl, emulate=False):
    """The reference's _generic_step (oracle/step_ref.py generic_step) plus the two pseudo-label terms, restated."""
    from oracle.net2d_ref import net2d_forward
    from oracle.step_ref import cross_modal_loss

    w = torch.tensor(W, dtype=torch.float32)
    logs, total = {}, 0.0
    for dom, lam in (("source", 1.0), ("target", 0.1)):
        b = batch[dom]
        p2d, _, _, a2d = net2d_forward(sd2d, b, training=True, dropout_masks=None, emulate_bf16=emulate)
        p3d, _, a3d = net3d(b)
        x2, x3 = cross_modal_loss(p3d["seg_logit"], a2d["seg_logit_avg"], p2d["seg_logit"], a3d["seg_logit_point"])
        if dom == "source":
            logs["loss_segmentation"] = F.cross_entropy(p2d["seg_logit"], b["seg_label"], weight=w)
            logs["loss_segmentation_3d"] = F.cross_entropy(p3d["seg_logit"], b["seg_label"], weight=w)
            logs["xm_loss_src_2d"], logs["xm_loss_src_3d"] = x2, x3
            total = total + logs["loss_segmentation"] + logs["loss_segmentation_3d"] + lam * (x2 + x3)
        else:
            logs["pl_loss_tgt_2d"] = F.cross_entropy(p2d["seg_logit"], b["pseudo_label_2d"], ignore_index=-100)
            logs["pl_loss_tgt_3d"] = F.cross_entropy(p3d["seg_logit"], b["pseudo_label_3d"], ignore_index=-100)
            logs["xm_loss_tgt_2d"], logs["xm_loss_tgt_3d"] = x2, x3
            total = total + lam * (x2 + x3) + lambda_pl * (logs["pl_loss_tgt_2d"] + logs["pl_loss_tgt_3d"])
    return total, logs


@pytest.mark.parametrize("kind", ["fp16", "bf16"])
def test_step_with_pseudo_labels_vs_oracle(kind):
    """The set-up and the tolerances of test_full_step_losses_and_gradients_vs_oracle, with lambda_pl = 0.5."""
    from oracle.net3d_ref import Net3DSegRef

    dev = _dev()
    n2, n3 = _nets()
    ref3 = Net3DSegRef(6, True, NET3D)
    ref3.load_state_dict(n3.state_dict())
    sd2 = {k: v.clone().requires_grad_(v.dtype.is_floating_point and "running" not in k) for k, v in n2.state_dict().items()}
    sd2e = {k: v.detach().clone().requires_grad_(v.requires_grad) for k, v in sd2.items()}
    ref3e = copy.deepcopy(ref3)
    ref_total, ref_logs = _oracle_step(sd2, ref3, _batch(None), 0.5)
    ref_total.backward()
    scale = 1024.0 if kind == "fp16" else 1.0
    emu_total, emu_logs = _oracle_step(sd2e, ref3e, _batch(None), 0.5, emulate=torch.float16 if kind == "fp16" else torch.bfloat16)
    (emu_total * scale).backward()
    tm = _trainer(n2.to(dev), n3.to(dev), precision=kind, lambda_pl=0.5)
    total = tm.training_step(_batch(dev))
    (total * scale).backward()
    if scale != 1.0:
        for v in list(sd2e.values()) + list(ref3e.parameters()) + list(n2.parameters()) + list(n3.parameters()):
            if v.grad is not None:
                v.grad.div_(scale)
    assert set(tm.last_logs) == {f"train/{k}" for k in ref_logs} and len(ref_logs) == 8
    tol = {"loss_segmentation_3d": 1e-3, "pl_loss_tgt_3d": 1e-3}  # 3D-only terms: fp32 on both sides
    worst_loss = 0.0
    for k, v in ref_logs.items():
        got = tm.last_logs[f"train/{k}"].item()
        print(f"{k}: {got:.6f} oracle {v.item():.6f} emulating oracle {emu_logs[k].item():.6f}")
        assert abs(got - v.item()) < tol.get(k, 3e-2) * max(1.0, abs(v.item())), k
        worst_loss = max(worst_loss, abs(got - emu_logs[k].item()) / max(1.0, abs(emu_logs[k].item())))
    assert abs(total.item() - ref_total.item()) < 3e-2 * max(1.0, abs(ref_total.item()))
    assert worst_loss < 1e-4, worst_loss
    g3 = dict(ref3.named_parameters())
    worst = 0.0
    for name, p in n3.named_parameters():
        if p.grad is not None:
            t = g3[name].grad
            worst = max(worst, ((p.grad.cpu() - t).abs().max() / max(1.0, t.abs().max())).item())
    cos_e = []
    for name, p in n2.named_parameters():
        if p.grad is not None and sd2[name].grad.norm() >= 1e-2:  # tiny early-layer gradients are the noisiest in 16 bits
            cos_e.append((F.cosine_similarity(p.grad.cpu().flatten().double(), sd2e[name].grad.flatten().double(), dim=0).item(), name))
    print(f"3D gradients worst {worst:.2e}; 2D gradient cosine vs the emulating oracle min {min(cos_e)[0]:.4f}; loss terms {worst_loss:.2e}")
    assert worst < 5e-2, worst
    assert min(cos_e)[0] > 0.93, sorted(cos_e)[:3]


def test_joined_pass_equals_the_two_call_sequence(bf16_mode):
    """Tolerances of test_joint_domain_pass_equals_the_two_call_sequence, over the eight terms."""
    dev = _dev()
    n2, n3 = _nets(dev)
    two = _trainer(copy.deepcopy(n2), copy.deepcopy(n3), joint_domains=False, lambda_pl=0.5)
    one = _trainer(n2, n3, lambda_pl=0.5)
    two.training_step(_batch(dev, 2)).backward()
    one.training_step(_batch(dev, 2)).backward()
    assert len(two.last_logs) == 8 and set(PL_KEYS) <= set(two.last_logs) and set(one.last_logs) == set(two.last_logs)
    for k, v in two.last_logs.items():
        tol = 1e-5 if k.endswith("segmentation_3d") else 2e-3
        assert abs(one.last_logs[k].item() - v.item()) < tol * max(1.0, abs(v.item())), (k, one.last_logs[k].item(), v.item())
    for (name, p), (_, q) in zip(n3.named_parameters(), two.model["3d_net"].named_parameters()):
        if q.grad is not None:
            assert (p.grad - q.grad).abs().max() <= 2e-2 * max(1e-3, float(q.grad.abs().max())), name


def _terms(dev, cfg=CE, joint=True, **swap):
    n2, n3 = _nets(dev)
    mode = swap.pop("mode", "own")
    tm = _trainer(n2, n3, cfg, precision="bf16", lambda_pl=0.5, pseudo_labels=mode, joint_domains=joint)
    total = tm.training_step(_batch(dev, **swap))
    return {k: v.item() for k, v in tm.last_logs.items()}, total.item()


def test_ensemble_mode_uses_the_ensemble_array_for_both_heads():
    """The three arrays differ; "ensemble" must equal "own" on a batch whose 2D and 3D arrays ARE the ensemble array (same
    kernels on the same numbers: bit-identical), and differ from "own" on the batch as it is."""
    dev = _dev()
    own, _ = _terms(dev)
    ens, total_ens = _terms(dev, mode="ensemble")
    swapped, total_swapped = _terms(dev, pseudo_label_2d="pseudo_label_ensemble", pseudo_label_3d="pseudo_label_ensemble")
    assert ens == swapped and total_ens == total_swapped
    assert all(ens[k] != own[k] for k in PL_KEYS)
    # ... on the two-call path too
    ens2, _ = _terms(dev, joint=False, mode="ensemble")
    swapped2, _ = _terms(dev, joint=False, pseudo_label_2d="pseudo_label_ensemble", pseudo_label_3d="pseudo_label_ensemble")
    assert ens2 == swapped2


def test_a_registry_with_two_segmentation_entries_takes_the_fallback_branch():
    """0.5 * CE + 0.5 * CE is not a single cross_entropy entry: the source terms go through the registry on the source slice,
    the pseudo-label terms through cross_entropy_pair with an unlabelled head - the same rows, labels and row arithmetic."""
    dev = _dev()
    half = [dict(CE[0], weight=0.5), dict(CE[0], weight=0.5)]
    one, total_one = _terms(dev)
    two, total_two = _terms(dev, cfg=half)
    assert set(one) == set(two) and len(two) == 8
    for k in PL_KEYS:
        assert two[k] == one[k], k  # unlabelled head rows add exact zeros to nothing: bit-identical
    for k in one:
        assert abs(two[k] - one[k]) <= 1e-6 * max(1.0, abs(one[k])), k
    assert abs(total_two - total_one) <= 1e-5 * max(1.0, abs(total_one))


def test_lambda_pl_zero_is_the_step_without_the_option():
    dev = _dev()
    res = []
    for kw in (dict(), dict(lambda_pl=0.0, pseudo_labels="ensemble")):
        n2, n3 = _nets(dev)
        tm = _trainer(n2, n3, precision="bf16", **kw)
        total = tm.training_step(_batch(dev))
        total.backward()
        res.append((total.item(), dict(tm.last_logs), [p.grad.clone() for p in n3.parameters() if p.grad is not None]))
    (t0, logs0, g0), (t1, logs1, g1) = res
    assert len(logs1) == 6 and list(logs0) == list(logs1) and not any("pl_loss" in k for k in logs1)
    assert t0 == t1 and all(logs0[k].item() == logs1[k].item() for k in logs0)
    assert all(torch.equal(a, b) for a, b in zip(g0, g1))


@pytest.mark.parametrize("joint", [True, False])
def test_refusals_come_before_any_launch(joint):
    dev = _dev()
    n2, n3 = _nets(dev)
    tm = _trainer(n2, n3, precision="bf16", lambda_pl=0.5, joint_domains=joint)
    missing = _batch(dev, pseudo=False)
    with pytest.raises(KeyError, match="pselab_paths="):
        tm.training_step(missing)
    no3d = _batch(dev)
    no3d["target"]["pseudo_label_3d"] = []
    with pytest.raises(ValueError, match='pseudo_labels="ensemble"'):
        tm.training_step(no3d)
    short = _batch(dev)
    short["target"]["pseudo_label_2d"] = short["target"]["pseudo_label_2d"][:-1]
    with pytest.raises(ValueError, match="point rows"):
        tm.training_step(short)
    torch.cuda.synchronize()
    # the empty 3D list is no obstacle in ensemble mode, and a good step follows the refusals
    ens = _trainer(n2, n3, precision="bf16", lambda_pl=0.5, joint_domains=joint, pseudo_labels="ensemble")
    assert np.isfinite(ens.training_step(no3d).item())
    total = tm.training_step(_batch(dev))
    total.backward()
    torch.cuda.synchronize()
    assert np.isfinite(total.item()) and all(np.isfinite(tm.last_logs[k].item()) for k in PL_KEYS)


def test_a_target_batch_without_a_counted_label_adds_nothing():
    """Every pseudo label -100: the terms are 0 (not 0/0), the total is finite and the gradients are those of lambda_pl = 0."""
    dev = _dev()
    grads = []
    for lam in (0.5, 0.0):
        n2, n3 = _nets(dev)
        tm = _trainer(n2, n3, precision="bf16", lambda_pl=lam)
        b = _batch(dev)
        for k in ("pseudo_label_2d", "pseudo_label_3d", "pseudo_label_ensemble"):
            b["target"][k] = torch.full_like(b["target"][k], -100)
        total = tm.training_step(b)
        total.backward()
        assert np.isfinite(total.item())
        if lam:
            assert all(tm.last_logs[k].item() == 0.0 for k in PL_KEYS)
        grads.append([p.grad.clone() for p in n3.parameters() if p.grad is not None])
    for a, b in zip(*grads):
        assert torch.isfinite(a).all() and torch.allclose(a, b, rtol=1e-4, atol=1e-7)


def test_one_self_training_round_on_the_miniature_data(tmp_path):
    """export_pseudo_labels -> PreprocessedScenes(pselab_paths=) -> gpu_batch -> two fit_step calls with lambda_pl = 1."""
    from mm2d3d_amd import pselab
    from mm2d3d_amd.datasets import PreprocessedScenes
    from mm2d3d_amd.losses import Loss
    from mm2d3d_amd.optimizers import Optimizer
    from mm2d3d_amd.train import TrainModel

    dev = _dev()
    write_scenes(str(tmp_path), 6)
    ds = PreprocessedScenes("train_day", str(tmp_path), str(tmp_path), output_orig=True, **KW)
    n2, n3 = _nets(dev)
    trainer = TrainModel({"2d_net": n2, "3d_net": n3}, {"2d_net": Optimizer("adamw", lr=1e-3), "3d_net": Optimizer("adamw", lr=1e-3)},
                         Loss([{"name": "cross_entropy", "target": "segmentation", "args": {}}]),
                         dict(lambda_xm_src=1.0, lambda_xm_trg=0.1, gc_freeze=False, num_classes=6, lambda_pl=1.0))
    path = str(tmp_path / "round1.npy")
    pselab.export_pseudo_labels(trainer, ds, path, batch_size=4, device=dev)
    trainer.model.train()
    target = PreprocessedScenes("train_day", str(tmp_path), str(tmp_path), pselab_paths=path, **KW)
    before = [p.detach().clone() for p in trainer.model.parameters()]
    for src_idx, trg_idx in (([0, 1], [2, 3]), ([4, 5], [0, 1])):
        batch = {"source": ds.gpu_batch(src_idx, device=dev), "target": target.gpu_batch(trg_idx, device=dev)}
        assert batch["target"]["pseudo_label_3d"].shape == batch["target"]["pseudo_label_2d"].shape
        loss = trainer.fit_step(batch)
        assert np.isfinite(loss.item())
        for k in PL_KEYS:
            v = trainer.last_logs[k].item()
            assert np.isfinite(v) and v > 0.0, (k, v)
    trainer.drain()
    for net in ("2d_net", "3d_net"):
        moved = [not torch.equal(p.detach(), q) for (name, p), q in zip(trainer.model.named_parameters(), before) if name.startswith(net)]
        assert any(moved), net
    torch.cuda.synchronize()
