"""GPU time of the mean-teacher update (csrc/optim.hip k_ema_update, mm2d3d_amd/ema.py) and of the step with and without it.

Kernel cost, over the table of the ``bench.py`` default trainer (the two AdamW arenas and every floating-point buffer):

  A  ``WeightEMA.update()``: one launch, reads the teacher and the weights and writes the teacher, 12 B per element.
  B  torch ``ema.copy_(p)`` over the same arenas (the buffers are left out: one launch per buffer would time the launches):
     8 B per element, the streaming copy the device does anyway.

HIP events around every iteration, A and B alternating in one process after a warm-up of both; median, 10th / 90th percentile
and minimum over ``--iters`` (>= 200) iterations each.  The expectation is A = about 1.5 x B.  ``--arenas-only`` times A over a
table without the buffer rows (what the ~200 tiny rows and their part of the row lookup cost).

Step cost: ``fit_step`` with ``ema_decay=None`` against ``0.999`` on two trainers with the same seed, alternating, ``--steps``
steps each on the same rotating batches.  One JSON line per measurement, then a markdown table.

    python tools/bench_ema.py [--iters 200] [--steps 30] [--out profiles/ema/bench_ema.md]
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
    from mm2d3d_amd.ema import WeightEMA
    from mm2d3d_amd.synthetic import make_batch

    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="timed iterations of A and of B")
    ap.add_argument("--steps", type=int, default=30, help="timed fit_step calls per trainer (0: skip the step timing)")
    ap.add_argument("--scenes", type=int, default=8, help="scenes per domain")
    ap.add_argument("--arenas-only", action="store_true", help="also time A over a table without the buffer rows")
    ap.add_argument("--out", default=None, help="also write the markdown table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema: needs a GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    kw = {"precision": "fp16"}
    with_ema = bench.build_trainer(dev, train_kwargs=dict(kw, ema_decay=0.999))
    ema = with_ema.ema
    pairs = [(e, a["p"]) for _, a, e in ema._arenas]
    n_arena, n_buf = sum(p.numel() for _, p in pairs), sum(b.numel() for _, b, _ in ema._buffers)
    shape = dict(rows=ema._nrows, arenas=len(pairs), arena_elements=n_arena, buffers=len(ema._buffers), buffer_elements=n_buf,
                 workgroups=ema._nblocks)
    print(json.dumps(dict(what="table", **shape)), flush=True)

    def run_a():
        ema.update()

    def run_b():
        for e, p in pairs:
            e.copy_(p)

    variants = {"A": run_a, "B": run_b}
    names = {"A": "A mm_ema_update, one launch over {} rows".format(ema._nrows), "B": "B torch ema.copy_(p) over the {} arenas".format(len(pairs))}
    if args.arenas_only:
        bare = WeightEMA(with_ema.optimizers, [], 0.999)
        variants["A0"] = bare.update
        names["A0"] = "A0 mm_ema_update over the {} arena rows alone".format(bare._nrows)
    for _ in range(20):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    evs = {k: [] for k in variants}
    for _ in range(max(args.iters, 1)):
        for k, fn in variants.items():
            evs[k].append(_timed(fn))
    torch.cuda.synchronize()
    ema.reset()  # the copies made the teacher the student: say so to the step timing below too
    lines = ["| what | median ms | p10 | p90 | min | n |", "|---|---:|---:|---:|---:|---:|"]
    rows = {}
    for k in variants:
        rows[k] = _stats([a.elapsed_time(b) for a, b in evs[k]])
        nbytes = (12 if k != "B" else 8) * n_arena + (12 * n_buf if k == "A" else 0)
        rows[k]["GB_per_s"] = round(nbytes / (rows[k]["median_ms"] * 1e-3) / 1e9, 1)
        print(json.dumps(dict(what=names[k], bytes=nbytes, **rows[k])), flush=True)
        lines.append("| {} ({:.1f} MB, {GB_per_s} GB/s) | {median_ms} | {p10_ms} | {p90_ms} | {min_ms} | {n} |".format(names[k], nbytes / 1e6, **rows[k]))
    ratio = rows["A"]["median_ms"] / rows["B"]["median_ms"]
    print(json.dumps(dict(what="A over B, medians", ratio=round(ratio, 3))), flush=True)
    lines.append("| A over B (medians) | {:.3f} | | | | |".format(ratio))

    if args.steps > 0:
        B = args.scenes
        without = bench.build_trainer(dev, train_kwargs=dict(kw))  # the same seed: the same weights
        assert without.ema is None
        batches = [{"source": make_batch(2, B, "nuscenes", (302, 480), 6, device=dev, augment=True, first_scene=j * B),
                    "target": make_batch(3, B, "nuscenes", (302, 480), 6, device=dev, augment=True, first_scene=j * B)} for j in range(4)]
        sides = {"ema_decay=None": without, "ema_decay=0.999": with_ema}
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
            tm.drain()
            r = _stats([a.elapsed_time(b) for a, b in sev[k]])
            name = f"fit_step, {k} ({B} + {B} scenes, fp16)"
            print(json.dumps(dict(what=name, **r)), flush=True)
            lines.append("| {} | {median_ms} | {p10_ms} | {p90_ms} | {min_ms} | {n} |".format(name, **r))
        # the teacher must not touch the training: the same seeds and batches give the same weights on both sides - as far as the
        # step repeats itself at this size at all, which a third trainer without a teacher tells (after the timing, not beside it)
        again = bench.build_trainer(dev, train_kwargs=dict(kw))
        sides["again"], seq["again"] = again, 0
        nxt["again"] = next_batch("again")
        for _ in range(5 + args.steps):
            seeded("again")
            step("again")
        torch.cuda.synchronize()

        def worst(x, y):
            return max(float((a["p"] - b["p"]).abs().max()) for o, q in zip(x.optimizers, y.optimizers) for a, b in zip(o._arenas, q._arenas))

        print(json.dumps(dict(what="largest weight difference after the same seeded steps", with_against_without_teacher=worst(with_ema, without),
                              without_against_without=worst(again, without))), flush=True)
    table = "\n".join(lines)
    print(table, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
