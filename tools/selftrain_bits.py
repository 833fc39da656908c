"""Bits of the self-training step, for comparing two checkouts of this project (a refactor against its parent).

    python tools/selftrain_bits.py dump OUT.npz [--only SUBSTRING[,SUBSTRING...]] [--skip SUBSTRING[,SUBSTRING...]]
    python tools/selftrain_bits.py compare A.npz B.npz

``dump`` runs every self-training option combination, and every other optional term of the step alone and all of them together
(``lambda_coral``, ``lambda_adv``, ``fda_beta``, ``xm_window``), for three ``fit_step`` calls at the shapes of tests/test_gpu_teacher_step.py
(1 + 1 synthetic nuScenes scenes, 48x64 images, 6 classes, fp16, dropout 0, ``ema_decay`` 0.9, heads scaled by 4; fresh nets from
seed 0 per case) and stores, as raw bytes: per step the loss, every ``last_logs`` value and every tensor of the ``LAST`` dicts
(``last_teacher`` ... ``last_match``); after the last step every entry of the checkpoint's "state_dict" and "ema_state_dict", the
state of ``pl_adaptive`` and the discriminators' parameters of the checkpoint's "adversary".  Then the
``direct/`` group: the row kernels called through ``pselab.predict``, ``pselab.teacher_labels``, ``AdaptiveThreshold.update``,
``losses.cross_entropy_soft_pair`` and ``losses.target_entropy`` at sizes the tiny step never reaches (``DIRECT_SIZES``: a tile and a
row, the class maximum, more tiles than workgroups of both tile sizes), contiguous and as row-pitched views, every output and
gradient as raw bytes.  It uses only ``train_kwargs``, ``fit_step``, ``last_logs``, the ``last_*`` attributes,
``pl_adaptive.state_dict()``, ``checkpoint()``, ``load_checkpoint()`` and those public functions, so the same file runs in either
checkout (it imports the package of the checkout whose ``tools/`` it lies in: copy it there).  The ``agreement/`` cases and the
``agreement`` direct calls (``pl_agreement``, ``pselab.agreement_weights``, the pairs' row weights) exist from the commit that added
them on: against an older checkout dump both sides with ``--skip agreement``.  ``compare`` demands equal key lists
and equal bytes, prints the number of arrays and the total bytes, and exits 1 on any difference.  One process per dump; every case
leaves its captured 2D trunk behind (some GiB of the device each), so all cases do not fit one process: dump them in groups chosen
with ``--only`` / ``--skip`` (``batch/``, ``teacher/``, ...), one process and one file per group, and compare group by group.
"""
import argparse
import gc
import itertools
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W = [1.9241476, 1.0, 2.16763851, 2.78254323, 1.54875664, 1.85686537]
NET3D = dict(in_channels=3, m=16, full_scale=4096, num_planes=7)
CE = {"name": "cross_entropy", "target": "segmentation", "args": {"weight": W}}
REGISTRY = {"single": [CE], "two_entries": [dict(CE, weight=0.5), dict(CE, weight=0.5)]}
STEPS = 3
ADAPTIVE = dict(pl_threshold_momentum=0.5, pl_threshold_warmup=True)  # the thresholds bite from the first step
PRIOR = [0.3, 0.1, 0.2, 0.1, 0.2, 0.1]
AGREEMENT_BETA = 0.5
DIRECT_SIZES = ((129, 5), (1000, 32), (131201, 6), (300001, 6))  # (N, C)
LAST = ("last_teacher", "last_agreement", "last_coral", "last_adversary", "last_fda", "last_match")  # trainer attributes: dicts or None


def cases():
    """name -> (train_kwargs, registry, extras of the target batch, prefetch, checkpoint round trip after step 2)."""
    out = {}

    def add(name, kw, registry="single", extras=None, prefetch=False, resume=False):
        if kw.get("pl_threshold") == "adaptive":
            kw = dict(kw, **ADAPTIVE)
        out[name] = (kw, registry, extras, prefetch, resume)

    calls = {"joined": {}, "two_calls": dict(joint_domains=False)}
    for mode, (call, ckw), reg in itertools.product(("own", "ensemble"), calls.items(), REGISTRY):
        add(f"batch/hard/{mode}/{call}/{reg}", dict(lambda_pl=1.0, pseudo_labels=mode, **ckw), reg, "labels")
    for mode, thr, T in itertools.product(("own", "ensemble"), (None, 0.9), (1.0, 2.0)):
        add(f"batch/soft/{mode}/thr_{thr}/T_{T}", dict(lambda_pl=1.0, pseudo_labels=mode, pl_targets="soft", pl_threshold=thr, pl_temperature=T),
            extras="logits")
    teacher = dict(lambda_pl=1.0, pseudo_label_source="teacher")
    for targets, thresholds in (("hard", (None, 0.9, "median", "adaptive")), ("soft", (None, 0.9, "adaptive"))):
        for thr in thresholds:
            for mode in ("own", "ensemble"):
                add(f"teacher/{targets}/{mode}/thr_{thr}/joined", dict(teacher, pseudo_labels=mode, pl_targets=targets, pl_threshold=thr))
            add(f"teacher/{targets}/own/thr_{thr}/two_calls", dict(teacher, pl_targets=targets, pl_threshold=thr, joint_domains=False))
    add("teacher/hard/own/thr_None/prefetched", dict(teacher), prefetch=True)
    add("teacher/lambda_pl_0", dict(lambda_pl=0.0, pseudo_label_source="teacher", pl_threshold=0.9))
    add("teacher/hard/own/thr_adaptive/checkpoint_round_trip", dict(teacher, pl_threshold="adaptive"), resume=True)
    infomax = dict(lambda_minent=0.1, lambda_div=0.1)  # MinEnt / InfoMax on the target rows
    for (call, ckw), (prior, pkw) in itertools.product(calls.items(), (("uniform", {}), ("prior", dict(div_prior=PRIOR)))):
        add(f"infomax/{call}/{prior}", dict(infomax, **ckw, **pkw))
    add("infomax/joined/uniform/with_teacher_soft_adaptive", dict(teacher, **infomax, pl_targets="soft", pl_threshold="adaptive"))
    agree = dict(pl_agreement=AGREEMENT_BETA)  # pseudo-label losses weighted by 2D/3D agreement
    add("agreement/teacher/hard/own/joined", dict(teacher, **agree))
    add("agreement/teacher/hard/ensemble/thr_median/joined", dict(teacher, **agree, pseudo_labels="ensemble", pl_threshold="median"))
    add("agreement/teacher/hard/own/two_calls", dict(teacher, **agree, joint_domains=False))
    add("agreement/teacher/soft/ensemble/thr_adaptive/joined", dict(teacher, **agree, pseudo_labels="ensemble", pl_targets="soft", pl_threshold="adaptive"))
    add("agreement/batch/hard/own/joined", dict(lambda_pl=1.0, **agree), extras="labels")
    add("agreement/batch/soft/own/thr_0.9/T_2.0", dict(lambda_pl=1.0, **agree, pl_targets="soft", pl_threshold=0.9, pl_temperature=2.0),
        extras="logits")
    for (call, ckw), mode in itertools.product(calls.items(), ("log", "plain")):  # CORAL / LogCORAL of the two domains' logits
        add(f"coral/{mode}/{call}", dict(lambda_coral=0.5, coral=mode, **ckw))
    for (call, ckw), mode in itertools.product(calls.items(), ("selfinfo", "softmax")):  # the output adversary and its discriminators
        add(f"adv/{mode}/{call}", dict(lambda_adv=0.1, adv_input=mode, adv_lr=1e-2, **ckw))
    add("adv/selfinfo/joined/checkpoint_round_trip", dict(lambda_adv=0.1, adv_lr=1e-2), resume=True)
    for (call, ckw), r in itertools.product(calls.items(), (1, 2)):  # the dense cross-modal window
        add(f"xm_window/{r}/{call}", dict(xm_window=r, **ckw))
    everything = dict(lambda_pl=1.0, lambda_minent=0.1, lambda_coral=0.5, lambda_adv=0.1, adv_lr=1e-2, fda_beta=0.05, xm_window=2)
    for call, ckw in calls.items():
        add(f"fda/{call}", dict(fda_beta=0.05, **ckw))  # a band of 2 at 48 x 64
        add(f"everything/{call}", dict(everything, **ckw), extras="labels")
    add("everything/joined/prefetched", dict(everything), extras="labels", prefetch=True)
    return out


def _trainer(dev, kw, registry):
    import torch

    from mm2d3d_amd.losses import Loss
    from mm2d3d_amd.net2d import Net2DSeg
    from mm2d3d_amd.net3d import Net3DSeg
    from mm2d3d_amd.optimizers import Optimizer
    from mm2d3d_amd.train import TrainModel

    torch.manual_seed(0)
    n2, n3 = Net2DSeg(6, pretrained=False), Net3DSeg(6, True, NET3D)
    for m in n2.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    with torch.no_grad():
        n2.con1_1_avg.weight.mul_(4.0), n3.linear.weight.mul_(4.0)
    return TrainModel({"2d_net": n2.to(dev), "3d_net": n3.to(dev)}, {k: Optimizer("adamw", lr=1e-3) for k in ("2d_net", "3d_net")},
                      Loss(REGISTRY[registry]), dict(lambda_xm_src=1.0, lambda_xm_trg=0.1, gc_freeze=False, precision="fp16", ema_decay=0.9, **kw))


def _batch(dev, extras, step):
    import torch

    from mm2d3d_amd.synthetic import make_batch

    b = {"source": make_batch(5, 1, "nuscenes", (48, 64), device=dev), "target": make_batch(6, 1, "nuscenes", (48, 64), device=dev)}
    n = int(b["target"]["x"][0].shape[0])
    g = torch.Generator().manual_seed(50 + step)
    if extras == "labels":  # as tests/test_gpu_pl_step.py _pseudo: about half are -100; the three arrays differ
        for k in ("pseudo_label_2d", "pseudo_label_3d", "pseudo_label_ensemble"):
            y = torch.randint(0, 6, (n,), generator=g)
            y[torch.rand(n, generator=g) < 0.5] = -100
            b["target"][k] = y.to(dev)
    elif extras == "logits":  # a frozen teacher of the caller's own: confidences on both sides of 0.9
        for k in ("teacher_logit_2d", "teacher_logit_3d"):
            b["target"][k] = (3.0 * torch.randn(n, 6, generator=g)).to(dev)
    return b


def _wanted(name, only, skip=None):
    if skip and any(part in name for part in skip.split(",")):
        return False
    return not only or any(part in name for part in only.split(","))


def _raw(t):
    import torch

    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy()


def _forget(tm):
    """Lets the trainer's device memory go (the optimisers' arenas and their hooks hold each other): forty trainers in one process."""
    import torch

    for opt in tm.optimizers:
        for a in getattr(opt, "_arenas", ()):
            if a is not None:
                a.clear()
    for q in tm.model.parameters():
        hooks = getattr(q, "_post_accumulate_grad_hooks", None)
        if hooks is not None:
            hooks.clear()
        q.__dict__.pop("_mm_hooks", None)
    gc.collect()
    torch.cuda.empty_cache()


def _direct_inputs(N, C, pitched, dev):
    """(student logits, teacher 2D, teacher 3D, head labels) of a size, seeded; two rows are not finite.  ``pitched``: each matrix
    a column slice of a wider NaN-filled one (stride(1) == 1, read in place)."""
    import torch

    g = torch.Generator().manual_seed(7000 + 37 * C + N % 1000)
    mats = [3.0 * torch.randn(N, C, generator=g) for _ in range(3)]
    mats[1][N - 2], mats[2][N - 2] = float("nan"), float("nan")  # a whole row of both teachers
    mats[1][N // 3, 1], mats[0][N - 1, 0] = float("inf"), float("inf")  # one entry of one teacher; one of the student's target rows
    y = torch.randint(0, C, (N,), generator=g)
    y[torch.rand(N, generator=g) < 0.3] = -100
    out = []
    for k, m in enumerate(mats):
        if pitched:
            wide = torch.full((N, C + 3 + k), float("nan"))
            wide[:, 1 + k : 1 + k + C] = m
            m = wide.to(dev)[:, 1 + k : 1 + k + C]
        out.append(m.to(dev))
    return out[0], out[1], out[2], y.to(dev)


def direct_cases(put, dev, only=None, skip=None):
    """The ``direct/`` group: every public entry of the row kernels at DIRECT_SIZES."""
    import torch

    from mm2d3d_amd import losses, pselab

    for (N, C), pitched in itertools.product(DIRECT_SIZES, (False, True)):
        base = f"direct/{N}_{C}/{'pitched' if pitched else 'contiguous'}"
        if not _wanted(base, only, skip):
            continue
        x, a, b, y = _direct_inputs(N, C, pitched, dev)
        P = N // 2
        thr2 = torch.linspace(0.35, 0.8, 2 * C, dtype=torch.float32, device=dev).reshape(2, C)
        prior = [1.0 + c for c in range(C)]

        def put_all(name, d):
            for k, v in d.items():
                if torch.is_tensor(v):
                    put(f"{base}/{name}/{k}", _raw(v))

        put_all("predict/2d", pselab.predict(a))
        put_all("predict/pair", pselab.predict(a, b))
        for ens in (False, True):
            for tname, thr in (("scalar", 0.6), ("per_class", thr2)):
                put_all(f"teacher_labels/ens_{ens}/{tname}", pselab.teacher_labels(a, b, ensemble=ens, threshold=thr, with_probs=True))
            ad = pselab.AdaptiveThreshold(C, momentum=0.5, warmup=True, device=dev)
            for k, lo in enumerate((0, N // 7, N // 3)):  # three updates in a row, different rows each time
                put(f"{base}/adaptive_update/ens_{ens}/thr{k}", _raw(ad.update(a[lo:], b[lo:], ensemble=ens)))
            put_all(f"adaptive_update/ens_{ens}", dict(state=ad.state, count=ad.count))
            for (tname, thr), T in itertools.product((("scalar", 0.6), ("per_class", thr2[0].contiguous())), (1.0, 2.0)):
                xg = x.detach().requires_grad_(True)
                lh, lt, kept = losses.cross_entropy_soft_pair(xg, P, y[:P], a[P:], b[P:] if ens else None, temperature=T, threshold=thr)
                (grad,) = torch.autograd.grad(lh + lt, xg)
                put_all(f"soft_pair/ens_{ens}/{tname}/T_{T}", dict(head=lh, tail=lt, kept=kept, grad=grad))
        for first, (pname, pr) in itertools.product((0, P), (("uniform", None), ("prior", prior))):
            xg = x.detach().requires_grad_(True)
            ent, div, mass, count = losses.target_entropy(xg, first, pr)
            (grad,) = torch.autograd.grad(ent + 0.5 * div, xg)
            put_all(f"target_entropy/first_{first}/{pname}", dict(ent=ent, div=div, mass=mass, count=count, grad=grad))
        if _wanted(f"{base}/agreement", only, skip):  # the weights of the tail rows, then both pairs under them
            ag = pselab.agreement_weights(a[P:], b[P:], AGREEMENT_BETA)
            put_all("agreement/weights", ag)
            y1 = y[P:].roll(1)
            for tname, thr in (("scalar", 0.6), ("per_class", thr2[0].contiguous())):
                xg = x.detach().requires_grad_(True)
                lh, lt, kept = losses.cross_entropy_soft_pair(xg, P, y[:P], a[P:], b[P:], temperature=2.0, threshold=thr, row_weight=ag["weight"])
                (grad,) = torch.autograd.grad(lh + lt, xg)
                put_all(f"agreement/soft_pair/{tname}", dict(head=lh, tail=lt, kept=kept, grad=grad))
            xg = x.detach().requires_grad_(True)
            lh, lt = losses.cross_entropy_pair(xg, P, y[:P], y1, weight_head=prior, row_weight_tail=ag["weight"])
            (grad,) = torch.autograd.grad(lh + lt, xg)
            put_all("agreement/hard_pair", dict(head=lh, tail=lt, grad=grad))
        torch.cuda.synchronize()
        print(f"{base}: done", flush=True)


def dump(path, only=None, skip=None):
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("selftrain_bits: needs a GPU")
    dev = torch.device("cuda:0")
    count = nbytes = 0
    archive = zipfile.ZipFile(path, "w", zipfile.ZIP_STORED, allowZip64=True)  # what np.savez writes, one array at a time

    def put(key, arr):
        nonlocal count, nbytes
        with archive.open(key + ".npy", "w", force_zip64=True) as f:
            np.lib.format.write_array(f, arr, allow_pickle=False)
        count, nbytes = count + 1, nbytes + arr.nbytes

    for name, (kw, registry, extras, prefetch, resume) in cases().items():
        if not _wanted(name, only, skip):
            continue
        tm = _trainer(dev, kw, registry)
        batches = [_batch(dev, extras, s) for s in range(STEPS)]
        for s in range(STEPS):
            if resume and s == 2:  # a fresh trainer takes over from the checkpoint, before its first teacher pass
                ckpt, old = tm.checkpoint(), tm
                tm = _trainer(dev, kw, registry)
                tm.load_checkpoint(ckpt)
                _forget(old)
            torch.manual_seed(100 + s)
            loss = tm.fit_step(batches[s], **(dict(next_batch=batches[s + 1]) if prefetch and s + 1 < STEPS else {}))
            put(f"{name}/step{s}/loss", _raw(loss))
            for k, v in tm.last_logs.items():
                put(f"{name}/step{s}/logs/{k}", _raw(v))
            for attr in LAST:  # an attribute the checkout does not know yet counts as None
                for k, v in (getattr(tm, attr, None) or {}).items():
                    if torch.is_tensor(v):
                        put(f"{name}/step{s}/{attr}/{k}", _raw(v))
        ckpt = tm.checkpoint()
        for part in ("state_dict", "ema_state_dict"):
            for k, v in ckpt[part].items():
                put(f"{name}/{part}/{k}", _raw(v))
        if tm.pl_adaptive is not None:
            for k, v in tm.pl_adaptive.state_dict().items():
                put(f"{name}/pl_adaptive/{k}", _raw(v) if torch.is_tensor(v) else np.array([v], dtype=np.int64).view(np.uint8))
        for i, p in enumerate((ckpt.get("adversary") or {}).get("params", ())):
            put(f"{name}/adversary/params{i}", _raw(p))
        torch.cuda.synchronize()
        print(f"{name}: loss {float(loss.detach()):.6f}, {len(tm.last_logs)} logged keys, "
              f"last_teacher {sorted(tm.last_teacher) if tm.last_teacher else None}", flush=True)
        _forget(tm)
        del tm, ckpt, batches
    direct_cases(put, dev, only, skip)
    archive.close()
    print(f"{count} arrays, {nbytes} bytes -> {path}", flush=True)


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    ka, kb = list(a.files), list(b.files)
    bad = []
    if ka != kb:
        bad += [f"only in {a_path}: {k}" for k in ka if k not in set(kb)] + [f"only in {b_path}: {k}" for k in kb if k not in set(ka)]
        bad += ["the key lists differ in order"] if not bad else []
    total = 0
    for k in ka:
        if k in b.files:
            x, y = a[k], b[k]
            total += x.nbytes
            if x.shape != y.shape or not np.array_equal(x, y):
                bad.append(f"differs: {k} ({x.nbytes} / {y.nbytes} bytes)")
    names = sorted({k.split("/step")[0] for k in ka if "/step" in k})
    direct = sorted({"/".join(k.split("/")[:4]) for k in ka if k.startswith("direct/")})
    print(f"{len(names)} step cases, {len(direct)} direct calls, {len(ka)} arrays, {total} bytes: "
          + ("all identical" if not bad else f"{len(bad)} DIFFERENCES"))
    for line in bad[:200]:
        print(line)
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("dump")
    d.add_argument("out")
    d.add_argument("--only", default=None, help="run the cases whose name contains one of these (comma-separated)")
    d.add_argument("--skip", default=None, help="leave out the cases and direct calls whose name contains one of these (comma-separated)")
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    args = ap.parse_args()
    if args.cmd == "dump":
        dump(args.out, args.only, args.skip)
    else:
        raise SystemExit(compare(args.a, args.b))


if __name__ == "__main__":
    main()
