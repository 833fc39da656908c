"""GPU time of the correlation-alignment loss of one head of the joined step, and of the step with and without it.

Shape: the rows of one head on the benchmark workload - the joined point count of ``make_batch`` for 8 + 8 scenes
(bench.py --workload c2: N = 558,080, P = 279,040); rows [0, P) are the source's, rows [P, N) the target's; x = 3 * randn mixed by a
random d x d matrix.

  (a) ``losses.coral`` at d = 6 (the class logits), mode "log" and mode "plain": two forward launches, one backward launch.
  (b) the same at d = 32, the widest rows the kernels take: what the in-kernel Jacobi finish costs at its cap.

Forward plus backward, HIP events around every iteration, the two modes alternating in one process after a warm-up of both;
median, 10th / 90th percentile and minimum over ``--iters`` (>= 200) iterations each.

  (c) ``fit_step`` on those batches with ``lambda_coral`` 0 against 1.0, alternating on one trainer.

One JSON line per measurement, then a markdown table.

    python tools/bench_coral.py [--iters 200] [--steps 30] [--out profiles/coral/bench_coral.md]

Launch counts come from a kernel trace taken in a run of its own (tracing slows the host), of one variant alone:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bench_coral.py --only log --iters 20

dispatches of that run, less those of the same run with ``--iters 0``, over 20 (tools/bench_pl_loss.py --count sums them).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("log", "plain")
ON = 1.0  # lambda_coral of the "on" side of the step timing


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

    from mm2d3d_amd.losses import coral
    from mm2d3d_amd.synthetic import make_batch

    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="timed iterations of each mode at each width")
    ap.add_argument("--steps", type=int, default=30, help="timed fit_step calls per side (0: skip the step timing)")
    ap.add_argument("--scenes", type=int, default=8, help="scenes per domain")
    ap.add_argument("--only", choices=MODES, default=None, help="run --iters iterations of one mode at d = 6 alone (for a kernel trace)")
    ap.add_argument("--out", default=None, help="also write the markdown table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_coral: needs a GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    B = args.scenes
    mk = lambda j: {"source": make_batch(2, B, "nuscenes", (302, 480), 6, device=dev, augment=True, first_scene=j * B),
                    "target": make_batch(3, B, "nuscenes", (302, 480), 6, device=dev, augment=True, first_scene=j * B)}
    first = mk(0)
    P = int(first["source"]["x"][0].shape[0])
    N = P + int(first["target"]["x"][0].shape[0])
    gen = torch.Generator().manual_seed(5)

    def rows(d):
        x = 3 * torch.randn(N, d, generator=gen) @ (torch.randn(d, d, generator=gen) / d ** 0.5)
        x[P:] *= 1.5
        return x.to(dev).requires_grad_(True)

    def run(x, mode):
        x.grad = None
        out = coral(x, P, mode)
        out["loss"].backward()
        return out["loss"]

    if args.only:
        x = rows(6)
        for _ in range(args.iters):
            run(x, args.only)
        torch.cuda.synchronize()
        print(json.dumps(dict(what=f"{args.only} alone", iters=args.iters, N=N, P=P)))
        return

    lines = ["| what | median ms | p10 | p90 | min | n |", "|---|---:|---:|---:|---:|---:|"]
    for d in (6, 32):
        x = rows(d)
        for _ in range(20):
            for mode in MODES:
                run(x, mode)
        torch.cuda.synchronize()
        evs = {m: [] for m in MODES}
        for _ in range(max(args.iters, 1)):
            for mode in MODES:
                evs[mode].append(_timed(lambda: run(x, mode)))
        torch.cuda.synchronize()
        for mode in MODES:
            r = _stats([a.elapsed_time(b) for a, b in evs[mode]])
            name = f"losses.coral, mode {mode}, d = {d}, forward + backward"
            print(json.dumps(dict(what=name, N=N, P=P, d=d, loss=float(run(x, mode)), **r)), flush=True)
            lines.append("| {} (N = {}, P = {}) | {median_ms} | {p10_ms} | {p90_ms} | {min_ms} | {n} |".format(name, N, P, **r))
        del x

    if args.steps > 0:
        import bench

        tm = bench.build_trainer(dev, train_kwargs={"precision": "fp16", "lambda_coral": ON})
        batches = [first] + [mk(j) for j in range(1, 4)]
        seq = [0]

        def next_batch():
            seq[0] += 1
            return bench.fresh(batches[(seq[0] - 1) % len(batches)])

        def step(on, cur, nxt):
            tm.lambda_coral = ON if on else 0.0  # read once per step by _generic_step: the same trainer and weights serve both sides
            return tm.fit_step(cur, next_batch=nxt)

        nxt = next_batch()
        for i in range(8):
            cur, nxt = nxt, next_batch()
            step(i % 2, cur, nxt)
        torch.cuda.synchronize()
        sev = {0: [], 1: []}
        for i in range(2 * args.steps):
            cur, nxt = nxt, next_batch()
            on = i % 2
            sev[on].append(_timed(lambda: step(on, cur, nxt)))
        torch.cuda.synchronize()
        tm.drain()
        for on in (0, 1):
            r = _stats([a.elapsed_time(b) for a, b in sev[on]])
            name = f"fit_step, lambda_coral = {ON if on else 0:g} (8 + 8 scenes, fp16, mode log)"
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
