"""GPU time of the pseudo-label losses weighted by 2D/3D agreement (csrc/pselab.hip k_pl_agree, csrc/loss.hip k_ce_*<2, RW> /
k_ce2s_*<.., RW>; pselab.agreement_weights, losses.cross_entropy_pair(row_weight_tail=), cross_entropy_soft_pair(row_weight=)) and
of the step that uses them.

Kernels, at one head's rows of the ``bench.py`` default workload, N = 558,080 joined points, P = 279,040, C = 6 (``--rows`` /
``--split`` / ``--classes``), the weights of the N - P tail rows from two teacher matrices, then forward plus backward of
``loss_head + loss_tail``:

  A  ``agreement_weights`` (two launches) plus the weighted pair: one forward launch (plus its finalize) and one backward launch.
  B  the same quantities composed from torch ops: two softmaxes and two log-softmaxes for ``D`` and ``w``; ``losses.cross_entropy`` on
     the head slice; on the tail slice ``F.cross_entropy(reduction="none")`` (hard) or ``-(q * log_softmax(x)).sum(1)`` under the
     confidence mask (soft) times ``w``, over the parents' denominators; autograd assembles the gradient of ``pred`` from the slices.

Once with hard tail labels (30 % of them -100) and once with the soft ensemble tail (``--temperature``, ``--threshold``).

Full step: ``fit_step`` with ``lambda_pl=1``, ``ema_decay=0.999``, ``pseudo_label_source="teacher"`` and hard targets on ONE trainer,
``pl_agreement`` alternating between None and ``--beta`` from step to step, ``--steps`` steps of each on the rotating batches of the
``bench.py`` default workload.

HIP events around every iteration, A and B alternating in one process after a warm-up of both; median, 10th / 90th percentile and
minimum.  One JSON line per measurement, then a markdown table.

    python tools/bench_agreement.py [--iters 200] [--steps 30] [--out profiles/agreement/bench_agreement.md]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(ms):
    return dict(median_ms=round(float(np.median(ms)), 4), p10_ms=round(float(np.percentile(ms, 10)), 4),
                p90_ms=round(float(np.percentile(ms, 90)), 4), min_ms=round(float(np.min(ms)), 4), n=len(ms))


def _timed(fn):
    import torch

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    return ev


def main():
    import torch
    import torch.nn.functional as F

    import bench
    from mm2d3d_amd import losses, pselab
    from mm2d3d_amd.synthetic import make_batch

    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="timed iterations of A and of B (0: skip the kernel timing)")
    ap.add_argument("--steps", type=int, default=30, help="timed fit_step calls per setting (0: skip the step timing)")
    ap.add_argument("--rows", type=int, default=558080, help="N: rows of one head's joined logits")
    ap.add_argument("--split", type=int, default=279040, help="P: the source rows")
    ap.add_argument("--classes", type=int, default=6)
    ap.add_argument("--beta", type=float, default=1.0)
    ap.add_argument("--temperature", type=float, default=2.0)
    ap.add_argument("--threshold", type=float, default=0.6)
    ap.add_argument("--scenes", type=int, default=8, help="scenes per domain")
    ap.add_argument("--out", default=None, help="also write the markdown table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_agreement: needs a GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    lines = ["| what | median ms | p10 | p90 | min | n |", "|---|---:|---:|---:|---:|---:|"]

    def table(name, r):
        print(json.dumps(dict(what=name, **r)), flush=True)
        lines.append("| {} | {median_ms} | {p10_ms} | {p90_ms} | {min_ms} | {n} |".format(name, **r))

    if args.iters > 0:
        N, P, C, T, thr, beta = args.rows, args.split, args.classes, args.temperature, args.threshold, args.beta
        g = torch.Generator().manual_seed(1234)
        x = (3.0 * torch.randn(N, C, generator=g)).to(dev).requires_grad_(True)
        ta, tb = (3.0 * torch.randn(N - P, C, generator=g)).to(dev), (3.0 * torch.randn(N - P, C, generator=g)).to(dev)
        y = torch.randint(0, C, (P,), generator=g).to(dev)
        y1 = torch.randint(0, C, (N - P,), generator=g)
        y1[torch.rand(N - P, generator=g) < 0.3] = -100
        y1 = y1.to(dev)
        cw = [1.9241476, 1.0, 2.16763851, 2.78254323, 1.54875664, 1.85686537][:C] + [1.0] * max(C - 6, 0)
        t = torch.tensor(thr, dtype=torch.float32, device=dev)
        res = {}

        def torch_weights():
            lp, lq = torch.log_softmax(ta, 1), torch.log_softmax(tb, 1)
            d = 0.5 * ((lp.exp() - lq.exp()) * (lp - lq)).sum(1)
            return torch.exp(-beta * d)

        def hard_a():
            x.grad = None
            w = pselab.agreement_weights(ta, tb, beta)["weight"]
            lh, lt = losses.cross_entropy_pair(x, P, y, y1, weight_head=cw, row_weight_tail=w)
            (lh + lt).backward()
            res["hard A"] = (lh.detach(), lt.detach(), x.grad)

        def hard_b():
            x.grad = None
            w = torch_weights()
            lh = losses.cross_entropy(x[:P], y, cw)
            valid = y1 != -100
            nll = F.cross_entropy(x[P:], y1, ignore_index=-100, reduction="none")
            lt = (w * nll)[valid].sum() / valid.sum()
            (lh + lt).backward()
            res["hard B"] = (lh.detach(), lt.detach(), x.grad)

        def soft_a():
            x.grad = None
            w = pselab.agreement_weights(ta, tb, beta)["weight"]
            lh, lt, kept = losses.cross_entropy_soft_pair(x, P, y, ta, tb, weight_head=cw, temperature=T, threshold=thr, row_weight=w)
            (lh + lt).backward()
            res["soft A"] = (lh.detach(), lt.detach(), x.grad)

        def soft_b():
            x.grad = None
            w = torch_weights()
            lh = losses.cross_entropy(x[:P], y, cw)
            mask = (0.5 * (torch.softmax(ta, 1) + torch.softmax(tb, 1))).max(1).values >= t
            q = 0.5 * (torch.softmax(ta / T, 1) + torch.softmax(tb / T, 1))
            lt = (w * -(q * torch.log_softmax(x[P:], 1)).sum(1))[mask].sum() / mask.sum()
            (lh + lt).backward()
            res["soft B"] = (lh.detach(), lt.detach(), x.grad)

        shape = f"N = {N}, P = {P}, C = {C}, beta = {beta}"
        names = {"hard A": f"A agreement_weights + cross_entropy_pair(row_weight_tail), forward + backward ({shape})",
                 "hard B": "B the same from torch ops: weights, cross_entropy on the head slice, weighted F.cross_entropy on the tail slice",
                 "soft A": f"A agreement_weights + cross_entropy_soft_pair(row_weight), forward + backward ({shape}, T = {T}, threshold {thr}, ensemble)",
                 "soft B": "B the same from torch ops: weights, cross_entropy on the head slice, masked weighted soft cross entropy on the tail slice"}
        for kind, variants in (("hard", {"hard A": hard_a, "hard B": hard_b}), ("soft", {"soft A": soft_a, "soft B": soft_b})):
            for _ in range(20):
                for fn in variants.values():
                    fn()
            torch.cuda.synchronize()
            a, b = res[kind + " A"], res[kind + " B"]
            agree = dict(head=abs(float(a[0]) - float(b[0])), tail=abs(float(a[1]) - float(b[1])), grad_max_abs_diff=float((a[2] - b[2]).abs().max()))
            print(json.dumps(dict(what=f"{kind}: A against B", **agree)), flush=True)
            assert agree["head"] < 1e-4 and agree["tail"] < 1e-4  # the same losses up to fp32 rounding, or no comparison
            evs = {k: [] for k in variants}
            for _ in range(args.iters):
                for k, fn in variants.items():
                    evs[k].append(_timed(fn))
            torch.cuda.synchronize()
            rows = {k: _stats([u.elapsed_time(v) for u, v in evs[k]]) for k in variants}
            for k in variants:
                table(names[k], rows[k])
            ratio = rows[kind + " B"]["median_ms"] / rows[kind + " A"]["median_ms"]
            print(json.dumps(dict(what=f"{kind}: B over A, medians", ratio=round(ratio, 3))), flush=True)
            lines.append("| {}: B over A (medians) | {:.3f} | | | | |".format(kind, ratio))
        ev = []
        for _ in range(args.iters):
            ev.append(_timed(lambda: pselab.agreement_weights(ta, tb, beta)))
        torch.cuda.synchronize()
        table(f"agreement_weights alone ({N - P} rows, C = {C})", _stats([u.elapsed_time(v) for u, v in ev]))

    if args.steps > 0:
        B = args.scenes
        kw = {"precision": "fp16", "ema_decay": 0.999, "lambda_pl": 1.0, "pseudo_label_source": "teacher"}
        tm = bench.build_trainer(dev, train_kwargs=kw)
        batches = [{"source": make_batch(2, B, "nuscenes", (302, 480), 6, device=dev, augment=True, first_scene=j * B),
                    "target": make_batch(3, B, "nuscenes", (302, 480), 6, device=dev, augment=True, first_scene=j * B)} for j in range(4)]
        print(json.dumps(dict(what="workload", scenes=f"{B} + {B}", target_rows=[int(bt["target"]["x"][0].shape[0]) for bt in batches])), flush=True)
        seq = [0]

        def next_batch():
            seq[0] += 1
            return bench.fresh(batches[(seq[0] - 1) % len(batches)])

        nxt = [next_batch()]

        def step(beta):
            tm.pl_agreement = beta  # forwarded to the SelfTraining policy: consulted anew by every step
            cur, nxt[0] = nxt[0], next_batch()
            torch.manual_seed(1000 + seq[0])
            return tm.fit_step(cur, next_batch=nxt[0])

        settings = {"pl_agreement=None": None, f"pl_agreement={args.beta}": args.beta}
        for _ in range(5):
            for beta in settings.values():
                step(beta)
        torch.cuda.synchronize()
        sev = {k: [] for k in settings}
        for _ in range(args.steps):
            for k, beta in settings.items():
                sev[k].append(_timed(lambda: step(beta)))
        torch.cuda.synchronize()
        for k in settings:
            table(f"fit_step GPU time, lambda_pl=1, teacher source, hard targets, {k} ({B} + {B} scenes, fp16)",
                  _stats([u.elapsed_time(v) for u, v in sev[k]]))
        logs = tm.last_logs
        print(json.dumps(dict(what="last step", **{n.split("/")[1]: float(logs[n].detach()) for n in logs if "/pl_" in n})), flush=True)
        tm.drain()
    out = "\n".join(lines)
    print(out, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
