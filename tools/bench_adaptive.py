"""GPU time of the self-adaptive per-class pseudo-label thresholds (csrc/pselab.hip k_pl_stats / k_pl_update and the per-class
k_teacher_labels; pselab.AdaptiveThreshold) and of the step that uses them.

Kernel cost, at the ``bench.py`` default's 279,040 target rows with 6 classes (``--rows`` / ``--classes``):

  A  ``AdaptiveThreshold.labels``: three launches - the statistics pass (reads both logit matrices), the one-workgroup update,
     and the label launch under the per-class thresholds (reads both matrices again, writes two int64 labels).
  B  ``pselab.teacher_labels(threshold=0.9)``: one launch, one hand-picked threshold.
  U  ``AdaptiveThreshold.update`` alone (what ``pl_targets="soft"`` adds: the loss calls read the thresholds themselves).

HIP events around every iteration, the variants alternating in one process after a warm-up of all; median, 10th / 90th
percentile and minimum over ``--iters`` iterations each.

Step cost: ``fit_step`` with ``lambda_pl=1``, ``ema_decay=0.999`` and ``pseudo_label_source="teacher"`` on two trainers with the same
seed, one with ``pl_threshold="adaptive"``, one with ``pl_threshold=0.9``, alternating, ``--steps`` steps each on the same rotating
batches of the ``bench.py`` default workload (the harness of tools/bench_teacher.py).  One JSON line per measurement, then a
markdown table.

    python tools/bench_adaptive.py [--iters 200] [--steps 30] [--out profiles/adaptive/bench_adaptive.md]
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
    from mm2d3d_amd import pselab
    from mm2d3d_amd.synthetic import make_batch

    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="timed iterations of every variant (0: skip the kernel timing)")
    ap.add_argument("--steps", type=int, default=30, help="timed fit_step calls per trainer (0: skip the step timing)")
    ap.add_argument("--rows", type=int, default=279040, help="target rows of the kernel timing")
    ap.add_argument("--classes", type=int, default=6)
    ap.add_argument("--scenes", type=int, default=8, help="scenes per domain")
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--momentum", type=float, default=0.999)
    ap.add_argument("--targets", default="hard", choices=("hard", "soft"), help="pl_targets of the step timing")
    ap.add_argument("--out", default=None, help="also write the markdown table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adaptive: needs a GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    lines = ["| what | median ms | p10 | p90 | min | n |", "|---|---:|---:|---:|---:|---:|"]

    if args.iters > 0:
        N, C, thr = args.rows, args.classes, args.threshold
        g = torch.Generator().manual_seed(1234)
        a, b = (3.0 * torch.randn(N, C, generator=g)).to(dev), (3.0 * torch.randn(N, C, generator=g)).to(dev)
        ad, upd = (pselab.AdaptiveThreshold(C, momentum=args.momentum, device=dev) for _ in range(2))
        res = {}

        def run_a():
            res["A"] = ad.labels(a, b)

        def run_b():
            res["B"] = pselab.teacher_labels(a, b, threshold=thr)

        def run_u():
            res["U"] = upd.update(a, b)

        variants = {"A": run_a, "B": run_b, "U": run_u}
        names = {"A": f"A AdaptiveThreshold.labels, three launches ({N} rows, C = {C}, momentum {args.momentum})",
                 "B": f"B pselab.teacher_labels, one launch, threshold {thr}",
                 "U": "U AdaptiveThreshold.update alone, two launches"}
        for _ in range(20):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        assert torch.equal(ad.state.view(torch.int64), upd.state.view(torch.int64))  # the same sequence, the same bits
        evs = {k: [] for k in variants}
        for _ in range(args.iters):
            for k, fn in variants.items():
                evs[k].append(_timed(fn))
        torch.cuda.synchronize()
        rows = {}
        for k in variants:
            rows[k] = _stats([x.elapsed_time(y) for x, y in evs[k]])
            print(json.dumps(dict(what=names[k], **rows[k])), flush=True)
            lines.append("| {} | {median_ms} | {p10_ms} | {p90_ms} | {min_ms} | {n} |".format(names[k], **rows[k]))
        print(json.dumps(dict(what="A over B, medians", ratio=round(rows["A"]["median_ms"] / rows["B"]["median_ms"], 3),
                              kept_A=res["A"]["kept"].tolist(), kept_B=res["B"]["kept"].tolist(),
                              tau=[round(float(v), 6) for v in ad.state[:, 0]], thr_2d=[round(float(v), 6) for v in res["A"]["threshold"][0]])),
              flush=True)
        lines.append("| A over B (medians) | {:.3f} | | | | |".format(rows["A"]["median_ms"] / rows["B"]["median_ms"]))

    if args.steps > 0:
        B = args.scenes
        kw = {"precision": "fp16", "ema_decay": 0.999, "lambda_pl": 1.0, "pseudo_label_source": "teacher", "pl_targets": args.targets}
        sides = {"pl_threshold=adaptive": bench.build_trainer(dev, train_kwargs=dict(kw, pl_threshold="adaptive", pl_threshold_momentum=args.momentum)),
                 f"pl_threshold={args.threshold}": bench.build_trainer(dev, train_kwargs=dict(kw, pl_threshold=args.threshold))}
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
            r = _stats([x.elapsed_time(y) for x, y in sev[k]])
            name = f"fit_step GPU time, lambda_pl=1, teacher source, pl_targets={args.targets}, {k} ({B} + {B} scenes, fp16)"
            print(json.dumps(dict(what=name, **r)), flush=True)
            lines.append("| {} | {median_ms} | {p10_ms} | {p90_ms} | {min_ms} | {n} |".format(name, **r))
            logs = tm.last_logs
            print(json.dumps(dict(what=f"last step, {k}", **{key.split("/")[1]: round(float(v.detach()), 6) for key, v in logs.items()
                                                              if "/pl_" in key})), flush=True)
            tm.drain()
    table = "\n".join(lines)
    print(table, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
