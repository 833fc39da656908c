"""GPU time of the online teacher labels (csrc/pselab.hip k_teacher_labels, pselab.teacher_labels) and of the step that uses them.

Kernel cost, at the ``bench.py`` default's 279,040 target rows with 6 classes (``--rows`` / ``--classes``):

  A  ``pselab.teacher_labels``: one launch, reads both logit matrices (2 x 4 C bytes per row) and writes two int64 labels.
  B  what the same labels cost before: ``pselab.predict`` (one launch, six outputs: three fp32 confidences and three uint8 labels
     per row) plus the torch ops that turn its outputs into thresholded int64 labels (two ``.long()``, two comparisons, two
     ``torch.where``) and the two kept counts.

HIP events around every iteration, A and B alternating in one process after a warm-up of both; median, 10th / 90th percentile
and minimum over ``--iters`` iterations each.

Step cost: ``fit_step`` with ``lambda_pl=1`` and ``ema_decay=0.999`` on two trainers with the same seed, one fed seeded labels in
the batch (``pseudo_label_source="batch"``), one labelling the batch itself (``"teacher"``), alternating, ``--steps`` steps each
on the same rotating batches of the ``bench.py`` default workload.  The difference is the teacher pass: two arena swaps, an eval
forward of the 2D net over the target images and of the 3D net over the joined rows, one label launch.  Host time is taken
afterwards, each side in a block of its own and every step from an empty queue (``--host-steps``), with the teacher pass and its
two eval-mode forwards timed beside it.  One JSON line per measurement, then a markdown table.

    python tools/bench_teacher.py [--iters 200] [--steps 30] [--out profiles/teacher/bench_teacher.md]

Launch counts: a kernel trace of one side alone, ``--iters 0 --host-steps 0 --sides teacher --steps N`` for two values of N; the
difference of the two runs' counts over the difference of N is the launches per step (tools/trace_counts.py).
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
    ap.add_argument("--iters", type=int, default=200, help="timed iterations of A and of B (0: skip the kernel timing)")
    ap.add_argument("--steps", type=int, default=30, help="timed fit_step calls per trainer (0: skip the step timing)")
    ap.add_argument("--host-steps", type=int, default=15, help="fit_step calls per trainer timed on the host, each from an empty queue")
    ap.add_argument("--sides", default="batch,teacher", help="which trainers to build (one alone: for a kernel trace of its launches)")
    ap.add_argument("--rows", type=int, default=279040, help="target rows of the kernel timing")
    ap.add_argument("--classes", type=int, default=6)
    ap.add_argument("--scenes", type=int, default=8, help="scenes per domain")
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--out", default=None, help="also write the markdown table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_teacher: needs a GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    lines = ["| what | median ms | p10 | p90 | min | n |", "|---|---:|---:|---:|---:|---:|"]

    if args.iters > 0:
        N, C, thr = args.rows, args.classes, args.threshold
        g = torch.Generator().manual_seed(1234)
        a, b = (3.0 * torch.randn(N, C, generator=g)).to(dev), (3.0 * torch.randn(N, C, generator=g)).to(dev)
        t = torch.tensor(thr, dtype=torch.float32, device=dev)
        ignore = torch.full((N,), -100, dtype=torch.int64, device=dev)
        res = {}

        def run_a():
            res["A"] = pselab.teacher_labels(a, b, threshold=thr)

        def run_b():
            r = pselab.predict(a, b)
            y2 = torch.where(r["probs_2d"] >= t, r["pseudo_label_2d"].long(), ignore)
            y3 = torch.where(r["probs_3d"] >= t, r["pseudo_label_3d"].long(), ignore)
            res["B"] = dict(label_2d=y2, label_3d=y3, kept=torch.stack([(y2 != -100).sum(), (y3 != -100).sum()]))

        variants = {"A": run_a, "B": run_b}
        names = {"A": f"A pselab.teacher_labels, one launch ({N} rows, C = {C}, threshold {thr})",
                 "B": "B pselab.predict + torch ops to the same int64 labels and counts"}
        for _ in range(20):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        assert all(torch.equal(res["A"][k], res["B"][k]) for k in ("label_2d", "label_3d", "kept"))  # the same labels, or no comparison
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
        nbytes = N * (2 * 4 * C + 2 * 8)
        ratio = rows["B"]["median_ms"] / rows["A"]["median_ms"]
        print(json.dumps(dict(what="B over A, medians", ratio=round(ratio, 3), A_bytes=nbytes,
                              A_GB_per_s=round(nbytes / (rows["A"]["median_ms"] * 1e-3) / 1e9, 1))), flush=True)
        lines.append("| B over A (medians); A moves {:.1f} MB | {:.3f} | | | | |".format(nbytes / 1e6, ratio))

    if args.steps > 0:
        import time

        B = args.scenes
        kw = {"precision": "fp16", "ema_decay": 0.999, "lambda_pl": 1.0}
        sides = {f"pseudo_label_source={k}": bench.build_trainer(dev, train_kwargs=dict(kw, pseudo_label_source=k))  # the same seed: the same weights
                 for k in args.sides.split(",")}
        batches = [{"source": make_batch(2, B, "nuscenes", (302, 480), 6, device=dev, augment=True, first_scene=j * B),
                    "target": make_batch(3, B, "nuscenes", (302, 480), 6, device=dev, augment=True, first_scene=j * B)} for j in range(4)]
        g = torch.Generator().manual_seed(77)
        for bt in batches:  # the batch source reads these; the teacher source ignores them
            n = int(bt["target"]["x"][0].shape[0])
            for k in ("pseudo_label_2d", "pseudo_label_3d"):
                bt["target"][k] = torch.randint(0, 6, (n,), generator=g).to(dev)
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
            name = f"fit_step GPU time, lambda_pl=1, {k} ({B} + {B} scenes, fp16)"
            print(json.dumps(dict(what=name, **r)), flush=True)
            lines.append("| {} | {median_ms} | {p10_ms} | {p90_ms} | {min_ms} | {n} |".format(name, **r))
        # Host time, each side in a block of its own and every step started on an EMPTY queue (a synchronise before it): the time
        # fit_step takes to return is then the host's own work plus its waits for this step's own read-backs, nothing of another
        # step's.  Eval-mode forwards of the two nets happen only inside the teacher pass: their host time is taken beside it.
        for k, tm in sides.items():
            acc = {}

            def wrap(name, net):
                orig = net.forward

                def fwd(*a, **kws):
                    if net.training:
                        return orig(*a, **kws)
                    t0 = time.perf_counter()
                    out = orig(*a, **kws)
                    acc[name] = acc.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
                    return out

                net.forward = fwd
                return orig

            origs = {name: wrap(name, net) for name, net in tm.model.items()}
            inner = tm.selftrain.teacher_targets

            def teacher_pass(*a, **kws):
                t0 = time.perf_counter()
                out = inner(*a, **kws)
                acc["teacher pass"] = acc.get("teacher pass", 0.0) + (time.perf_counter() - t0) * 1e3
                return out

            tm.selftrain.teacher_targets = teacher_pass
            host, wall, parts = [], [], []
            for _ in range(args.host_steps):
                seeded(k)
                acc.clear()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                step(k)
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                host.append((t1 - t0) * 1e3)
                wall.append((time.perf_counter() - t0) * 1e3)
                parts.append(dict(acc))
            del tm.selftrain.teacher_targets  # the instance attribute: the class's method is back
            for name, net in tm.model.items():
                del net.forward  # the instance attribute: the class's method is back
            if host:
                r = _stats(host)
                extra = {f"host_ms_{n.replace(' ', '_')}_median": round(float(np.median([p.get(n, 0.0) for p in parts])), 3)
                         for n in sorted({n for p in parts for n in p})}
                name = f"fit_step host time from an empty queue, {k}"
                print(json.dumps(dict(what=name, step_wall_median_ms=round(float(np.median(wall)), 3), **extra, **r)), flush=True)
                lines.append("| {} | {median_ms} | {p10_ms} | {p90_ms} | {min_ms} | {n} |".format(name, **r))
                lines.append("| ... the same steps, start to drained queue | {:.3f} | | | | |".format(float(np.median(wall))))
                for n, v in extra.items():
                    lines.append("| ... of the host time: {} | {:.3f} | | | | |".format(n[len("host_ms_"):-len("_median")].replace("_", " "), v))
            tm.drain()
        tk = sides.get("pseudo_label_source=teacher")
        if tk is not None:
            kept = tk.last_logs
            print(json.dumps(dict(what="last teacher step", pl_kept_2d=float(kept["train/pl_kept_2d"]), pl_kept_3d=float(kept["train/pl_kept_3d"]),
                                  pl_loss_tgt_2d=float(kept["train/pl_loss_tgt_2d"].detach()), pl_loss_tgt_3d=float(kept["train/pl_loss_tgt_3d"].detach()))), flush=True)
    table = "\n".join(lines)
    print(table, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
