"""GPU time of Fourier domain adaptation of the source images, and of the training step with and without it.

  (a) ``fda.fda_transfer`` alone at 8 + 8 images of 3 x 225 x 400 and of 3 x 302 x 480 (the loaders' sizes), ``beta`` 0.01 and
      0.09 (bands 2 / 20 and 3 / 27): three launches per call.  Source pixels uniform in 0..255, target pixels darker.

HIP events around every call, the variants alternating in one process after a warm-up of all; median, 10th / 90th percentile
and minimum over ``--iters`` (>= 200) calls each.

  (b) ``fit_step`` on the benchmark workload (bench.py --workload c2: 8 + 8 scenes, 302 x 480 images, fp16) with ``fda_beta`` None
      against 0.09, alternating on two trainers built alike.  The None side is the step without the option, launch for launch.

One JSON line per measurement, then a markdown table.

    python tools/bench_fda.py [--iters 200] [--steps 30] [--out profiles/fda/bench_fda.md]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((225, 400), (302, 480))
BETAS = (0.01, 0.09)
ON = 0.09  # fda_beta of the "on" side of the step timing


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

    from mm2d3d_amd.fda import fda_transfer
    from mm2d3d_amd.synthetic import make_batch

    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="timed calls of each variant")
    ap.add_argument("--steps", type=int, default=30, help="timed fit_step calls per side (0: skip the step timing)")
    ap.add_argument("--images", type=int, default=8, help="images per domain")
    ap.add_argument("--out", default=None, help="also write the markdown table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fda: needs a GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    B = args.images
    gen = torch.Generator().manual_seed(5)
    lines = ["| what | median ms | p10 | p90 | min | n |", "|---|---:|---:|---:|---:|---:|"]

    variants = {}
    for H, W in SIZES:
        src = (255.0 * torch.rand(B, 3, H, W, generator=gen)).to(dev)
        trg = (120.0 * torch.rand(B, 3, H, W, generator=gen) ** 2).to(dev)
        for beta in BETAS:
            variants[(H, W, beta)] = (src, trg)
    out = {}
    for _ in range(20):
        for (H, W, beta), (src, trg) in variants.items():
            out[(H, W, beta)] = fda_transfer(src, trg, beta)
    torch.cuda.synchronize()
    evs = {k: [] for k in variants}
    for _ in range(max(args.iters, 1)):
        for (H, W, beta), (src, trg) in variants.items():
            evs[(H, W, beta)].append(_timed(lambda: fda_transfer(src, trg, beta)))
    torch.cuda.synchronize()
    for (H, W, beta), pairs in evs.items():
        r = _stats([a.elapsed_time(b) for a, b in pairs])
        o = out[(H, W, beta)]
        name = f"fda_transfer, {B} + {B} images of 3 x {H} x {W}, beta {beta:g} (band {o['band']})"
        print(json.dumps(dict(what=name, H=H, W=W, beta=beta, band=o["band"], mse=float(o["mse"].mean()), **r)), flush=True)
        lines.append("| {} | {median_ms} | {p10_ms} | {p90_ms} | {min_ms} | {n} |".format(name, **r))
    del variants, out, evs

    if args.steps > 0:
        import bench

        mk = lambda j: {"source": make_batch(2, B, "nuscenes", (302, 480), 6, device=dev, augment=True, first_scene=j * B),
                        "target": make_batch(3, B, "nuscenes", (302, 480), 6, device=dev, augment=True, first_scene=j * B)}
        batches = [mk(j) for j in range(4)]
        sides = {}
        for on in (0, 1):
            tm = bench.build_trainer(dev, train_kwargs={"precision": "fp16", "fda_beta": ON if on else None})
            sides[on] = dict(tm=tm, seq=0, nxt=None)

        def next_batch(side):
            side["seq"] += 1
            return bench.fresh(batches[(side["seq"] - 1) % len(batches)])

        def step(side):
            cur, side["nxt"] = side["nxt"], next_batch(side)
            return side["tm"].fit_step(cur, next_batch=side["nxt"])

        for side in sides.values():
            side["nxt"] = next_batch(side)
        for i in range(10):
            step(sides[i % 2])
        torch.cuda.synchronize()
        sev = {0: [], 1: []}
        for i in range(2 * args.steps):
            on = i % 2
            sev[on].append(_timed(lambda: step(sides[on])))
        torch.cuda.synchronize()
        for on in (0, 1):
            sides[on]["tm"].drain()
            r = _stats([a.elapsed_time(b) for a, b in sev[on]])
            name = f"fit_step, fda_beta = {ON if on else None} ({B} + {B} scenes, 302 x 480 images, fp16)"
            print(json.dumps(dict(what=name, **r)), flush=True)
            lines.append("| {} | {median_ms} | {p10_ms} | {p90_ms} | {min_ms} | {n} |".format(name, **r))
    table = "\n".join(lines)
    print(table, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
