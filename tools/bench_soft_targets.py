"""GPU time of the soft mean-teacher targets (csrc/loss.hip k_ce2s_*, losses.cross_entropy_soft_pair) and of the step that uses them.

Loss call, at one head's rows of the ``bench.py`` default workload, N = 558,080 joined points, P = 279,040, C = 6 (``--rows`` /
``--split`` / ``--classes``), forward plus backward of ``loss_head + loss_tail``, ensemble target, ``--temperature``, ``--threshold``:

  A  ``cross_entropy_soft_pair``: one forward launch (plus its finalize) and one backward launch over all N rows.
  B  the composition possible without it: ``losses.cross_entropy`` on the head slice, plus torch ops on the tail slice - the two
     softmaxes at temperature 1 for the confidence mask, the two at T for ``q``, ``-(q * log_softmax(x)).sum(1)[mask].mean()`` -
     with autograd assembling the gradient of ``pred`` from the two slices.

Full step: ``fit_step`` with ``lambda_pl=1``, ``ema_decay=0.999`` and ``pseudo_label_source="teacher"`` on two trainers with the same
seed, A with ``pl_targets="soft"``, B with ``"hard"``, ``--steps`` steps each on the same rotating batches of the ``bench.py`` default
workload.

HIP events around every iteration, A and B alternating in one process after a warm-up of both; median, 10th / 90th percentile and
minimum.  One JSON line per measurement, then a markdown table.

    python tools/bench_soft_targets.py [--iters 200] [--steps 30] [--out profiles/soft_targets/bench_soft_targets.md]
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

    import bench
    from mm2d3d_amd import losses
    from mm2d3d_amd.synthetic import make_batch

    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="timed iterations of A and of B (0: skip the loss timing)")
    ap.add_argument("--steps", type=int, default=30, help="timed fit_step calls per trainer (0: skip the step timing)")
    ap.add_argument("--rows", type=int, default=558080, help="N: rows of one head's joined logits")
    ap.add_argument("--split", type=int, default=279040, help="P: the source rows")
    ap.add_argument("--classes", type=int, default=6)
    ap.add_argument("--temperature", type=float, default=2.0)
    ap.add_argument("--threshold", type=float, default=0.6)
    ap.add_argument("--scenes", type=int, default=8, help="scenes per domain")
    ap.add_argument("--out", default=None, help="also write the markdown table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_soft_targets: needs a GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    lines = ["| what | median ms | p10 | p90 | min | n |", "|---|---:|---:|---:|---:|---:|"]

    if args.iters > 0:
        N, P, C, T, thr = args.rows, args.split, args.classes, args.temperature, args.threshold
        g = torch.Generator().manual_seed(1234)
        x = (3.0 * torch.randn(N, C, generator=g)).to(dev).requires_grad_(True)
        ta, tb = (3.0 * torch.randn(N - P, C, generator=g)).to(dev), (3.0 * torch.randn(N - P, C, generator=g)).to(dev)
        y = torch.randint(0, C, (P,), generator=g).to(dev)
        w = [1.9241476, 1.0, 2.16763851, 2.78254323, 1.54875664, 1.85686537][:C] + [1.0] * max(C - 6, 0)
        t = torch.tensor(thr, dtype=torch.float32, device=dev)
        res = {}

        def run_a():
            x.grad = None
            lh, lt, kept = losses.cross_entropy_soft_pair(x, P, y, ta, tb, weight_head=w, temperature=T, threshold=thr)
            (lh + lt).backward()
            res["A"] = (lh.detach(), lt.detach(), kept, x.grad)

        def run_b():
            x.grad = None
            lh = losses.cross_entropy(x[:P], y, w)
            conf = (0.5 * (torch.softmax(ta, 1) + torch.softmax(tb, 1))).max(1).values
            mask = conf >= t
            q = 0.5 * (torch.softmax(ta / T, 1) + torch.softmax(tb / T, 1))
            lt = -(q * torch.log_softmax(x[P:], 1)).sum(1)[mask].mean()
            (lh + lt).backward()
            res["B"] = (lh.detach(), lt.detach(), mask.sum(), x.grad)

        variants = {"A": run_a, "B": run_b}
        names = {"A": f"A cross_entropy_soft_pair, forward + backward (N = {N}, P = {P}, C = {C}, T = {T}, threshold {thr}, ensemble)",
                 "B": "B cross_entropy on the head slice + torch ops on the tail slice, autograd assembling the gradient"}
        for _ in range(20):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        a, b = res["A"], res["B"]
        agree = dict(kept_A=int(a[2]), kept_B=int(b[2]), head=abs(float(a[0]) - float(b[0])), tail=abs(float(a[1]) - float(b[1])),
                     grad_max_abs_diff=float((a[3] - b[3]).abs().max()))
        print(json.dumps(dict(what="A against B", **agree)), flush=True)
        # the same losses and gradient up to fp32 rounding, or no comparison (a row whose confidence rounds across the threshold
        # in torch's softmax but not in the kernel's would move the count by one)
        assert abs(agree["kept_A"] - agree["kept_B"]) <= 2 and agree["head"] < 1e-4 and agree["tail"] < 1e-4
        evs = {k: [] for k in variants}
        for _ in range(args.iters):
            for k, fn in variants.items():
                evs[k].append(_timed(fn))
        torch.cuda.synchronize()
        rows = {}
        for k in variants:
            rows[k] = _stats([u.elapsed_time(v) for u, v in evs[k]])
            print(json.dumps(dict(what=names[k], **rows[k])), flush=True)
            lines.append("| {} | {median_ms} | {p10_ms} | {p90_ms} | {min_ms} | {n} |".format(names[k], **rows[k]))
        ratio = rows["B"]["median_ms"] / rows["A"]["median_ms"]
        print(json.dumps(dict(what="B over A, medians", ratio=round(ratio, 3))), flush=True)
        lines.append("| B over A (medians) | {:.3f} | | | | |".format(ratio))

    if args.steps > 0:
        B = args.scenes
        kw = {"precision": "fp16", "ema_decay": 0.999, "lambda_pl": 1.0, "pseudo_label_source": "teacher"}
        sides = {f"pl_targets={k}": bench.build_trainer(dev, train_kwargs=dict(kw, pl_targets=k)) for k in ("soft", "hard")}  # the same seed
        batches = [{"source": make_batch(2, B, "nuscenes", (302, 480), 6, device=dev, augment=True, first_scene=j * B),
                    "target": make_batch(3, B, "nuscenes", (302, 480), 6, device=dev, augment=True, first_scene=j * B)} for j in range(4)]
        print(json.dumps(dict(what="workload", scenes=f"{B} + {B}", target_rows=[int(bt["target"]["x"][0].shape[0]) for bt in batches])), flush=True)
        seq = {k: 0 for k in sides}
        nxt = {}

        def next_batch(k):
            seq[k] += 1
            return bench.fresh(batches[(seq[k] - 1) % len(batches)])

        def step(k):
            cur, nxt[k] = nxt[k], next_batch(k)
            return sides[k].fit_step(cur, next_batch=nxt[k])

        def seeded(k):
            torch.manual_seed(1000 + seq[k])  # the dropout masks draw from the global generator: step i gets the same ones on every side

        for k in sides:
            nxt[k] = next_batch(k)
        for _ in range(5):
            for k in sides:
                seeded(k)
                step(k)
        torch.cuda.synchronize()
        sev = {k: [] for k in sides}
        for _ in range(args.steps):
            for k in sides:
                seeded(k)
                sev[k].append(_timed(lambda: step(k)))
        torch.cuda.synchronize()
        for k, tm in sides.items():
            r = _stats([u.elapsed_time(v) for u, v in sev[k]])
            name = f"fit_step GPU time, lambda_pl=1, teacher source, {k} ({B} + {B} scenes, fp16)"
            print(json.dumps(dict(what=name, **r)), flush=True)
            lines.append("| {} | {median_ms} | {p10_ms} | {p90_ms} | {min_ms} | {n} |".format(name, **r))
            logs = tm.last_logs
            print(json.dumps(dict(what=f"last step, {k}", **{n.split("/")[1]: float(logs[n].detach()) for n in logs if "/pl_" in n})), flush=True)
            tm.drain()
    table = "\n".join(lines)
    print(table, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
