"""GPU time of the pseudo-label loss of one head of the joined step, and of the step with and without it.

Shape: the rows of one head on the benchmark workload - the joined point count of ``make_batch`` for 8 + 8 scenes
(bench.py --workload c2), C = 6; rows [0, P) are the source's (labels with 5 % ignored, the six class weights), rows [P, N) the
target's (pseudo labels with 50 % ignored, no weights).

  A  ``losses.cross_entropy_pair``: one forward call, one backward launch for both losses.
  B  the same two losses from the building blocks that were there before it: ``losses.cross_entropy`` on the two row slices,
     autograd assembling the gradient of the whole tensor (slice backward = zero fill + copy per slice, then an add).

Forward plus backward of ``loss_head + loss_tail``, HIP events around every iteration, A and B alternating in one process after
a warm-up of both; median, 10th / 90th percentile and minimum over ``--iters`` (>= 200) iterations each.  Then ``fit_step`` on
those batches with ``lambda_pl`` 0 against 1.0, alternating on one trainer.  One JSON line per measurement, then a markdown table.

    python tools/bench_pl_loss.py [--iters 200] [--steps 30] [--out profiles/pl_loss/bench_pl_loss.md]

Launch counts come from a kernel trace taken in a run of its own (tracing slows the host), of one variant alone:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_pl_loss.py --only A --iters 20

dispatches of that run, less those of the same run with ``--iters 0``, over 20 (no GPU needed for the sum):

    python tools/bench_pl_loss.py --count <dir> [--base <dir of the --iters 0 run>] --iters 20
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASS_WEIGHTS = [1.9241476, 1.0, 2.16763851, 2.78254323, 1.54875664, 1.85686537]
C = 6


def _labels(n, ignored, gen):
    import torch

    y = torch.randint(0, C, (n,), generator=gen)
    y[torch.rand(n, generator=gen) < ignored] = -100
    return y


def _stats(ms):
    return dict(median_ms=round(float(np.median(ms)), 4), p10_ms=round(float(np.percentile(ms, 10)), 4),
                p90_ms=round(float(np.percentile(ms, 90)), 4), min_ms=round(float(np.min(ms)), 4), n=len(ms))


def _count(trace_dir, base_dir, iters):
    """Kernel launches per iteration from the ``*kernel_stats.csv`` of two rocprofv3 runs (a run without kernels writes none)."""
    import csv
    import glob

    def calls(d):
        out = {}
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True) if d else []:
            for r in csv.DictReader(open(f)):
                out[r["Name"]] = out.get(r["Name"], 0) + int(r["Calls"])
        return out

    run, base = calls(trace_dir), calls(base_dir)
    if not run:
        raise SystemExit(f"bench_pl_loss: no *kernel_stats.csv under {trace_dir}")
    per = {k: (v - base.get(k, 0)) / iters for k, v in run.items() if v != base.get(k, 0)}
    print(json.dumps(dict(launches_per_iteration=round(sum(per.values()), 2), kernels=per), indent=1))


def _timed(fn):
    import torch

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    return ev


def main():
    import torch

    from mm2d3d_amd.losses import cross_entropy, cross_entropy_pair
    from mm2d3d_amd.synthetic import make_batch

    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="timed iterations of A and of B")
    ap.add_argument("--steps", type=int, default=30, help="timed fit_step calls per lambda_pl value (0: skip the step timing)")
    ap.add_argument("--scenes", type=int, default=8, help="scenes per domain")
    ap.add_argument("--only", choices=["A", "B"], default=None, help="run --iters iterations of one variant alone (for a kernel trace)")
    ap.add_argument("--count", metavar="DIR", default=None, help="sum the kernel trace under DIR into launches per iteration")
    ap.add_argument("--base", metavar="DIR", default=None, help="with --count: the trace of the same run with --iters 0")
    ap.add_argument("--out", default=None, help="also write the markdown table to this file")
    args = ap.parse_args()
    if args.count:
        return _count(args.count, args.base, max(args.iters, 1))
    if not torch.cuda.is_available():
        raise SystemExit("bench_pl_loss: needs a GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    B = args.scenes
    mk = lambda j: {"source": make_batch(2, B, "nuscenes", (302, 480), 6, device=dev, augment=True, first_scene=j * B),
                    "target": make_batch(3, B, "nuscenes", (302, 480), 6, device=dev, augment=True, first_scene=j * B)}
    first = mk(0)
    P = int(first["source"]["x"][0].shape[0])
    N = P + int(first["target"]["x"][0].shape[0])
    gen = torch.Generator().manual_seed(5)
    x = (3 * torch.randn(N, C, generator=gen)).to(dev).requires_grad_(True)
    y0, y1 = _labels(P, 0.05, gen).to(dev), _labels(N - P, 0.5, gen).to(dev)

    def run_a():
        x.grad = None
        lh, lt = cross_entropy_pair(x, P, y0, y1, weight_head=CLASS_WEIGHTS)
        (lh + lt).backward()
        return lh, lt

    def run_b():
        x.grad = None
        lh, lt = cross_entropy(x[:P], y0, CLASS_WEIGHTS), cross_entropy(x[P:], y1)
        (lh + lt).backward()
        return lh, lt

    if args.only:
        fn = run_a if args.only == "A" else run_b
        for _ in range(args.iters):
            fn()
        torch.cuda.synchronize()
        print(json.dumps(dict(what=f"{args.only} alone", iters=args.iters, N=N, P=P)))
        return

    # faster and different is not faster: the two variants compute the same numbers
    la, ga = [v.item() for v in run_a()], x.grad.clone()
    lb, gb = [v.item() for v in run_b()], x.grad.clone()
    diff = dict(loss_head=abs(la[0] - lb[0]), loss_tail=abs(la[1] - lb[1]), grad_max_abs=(ga - gb).abs().max().item())
    print(json.dumps(dict(what="A against B", N=N, P=P, **diff)), flush=True)
    assert diff["loss_head"] < 1e-5 and diff["loss_tail"] < 1e-5 and diff["grad_max_abs"] < 1e-9, diff
    for _ in range(20):
        run_a(), run_b()
    torch.cuda.synchronize()
    evs = {"A": [], "B": []}
    for _ in range(max(args.iters, 1)):
        evs["A"].append(_timed(run_a))
        evs["B"].append(_timed(run_b))
    torch.cuda.synchronize()
    lines = ["| what | median ms | p10 | p90 | min | n |", "|---|---:|---:|---:|---:|---:|"]
    rows = {}
    for k, name in (("A", "A cross_entropy_pair, forward + backward"), ("B", "B cross_entropy on two slices, forward + backward")):
        rows[k] = _stats([a.elapsed_time(b) for a, b in evs[k]])
        print(json.dumps(dict(what=name, N=N, P=P, C=C, **rows[k])), flush=True)
        lines.append("| {} (N = {}, P = {}) | {median_ms} | {p10_ms} | {p90_ms} | {min_ms} | {n} |".format(name, N, P, **rows[k]))

    if args.steps > 0:
        import bench

        tm = bench.build_trainer(dev, train_kwargs={"precision": "fp16", "lambda_pl": 1.0})
        batches = [first] + [mk(j) for j in range(1, 4)]
        for j, b in enumerate(batches):
            g = torch.Generator().manual_seed(100 + j)
            n = int(b["target"]["x"][0].shape[0])
            for k in ("pseudo_label_2d", "pseudo_label_3d", "pseudo_label_ensemble"):
                b["target"][k] = _labels(n, 0.5, g).to(dev)
        seq = [0]

        def next_batch():
            seq[0] += 1
            return bench.fresh(batches[(seq[0] - 1) % len(batches)])

        def step(lam, cur, nxt):
            tm.lambda_pl = lam  # read once per step by _generic_step: the same trainer and weights serve both sides
            return tm.fit_step(cur, next_batch=nxt)

        nxt = next_batch()
        for i in range(8):
            cur, nxt = nxt, next_batch()
            step(float(i % 2), cur, nxt)
        torch.cuda.synchronize()
        sev = {0.0: [], 1.0: []}
        for i in range(2 * args.steps):
            cur, nxt = nxt, next_batch()
            lam = float(i % 2)
            sev[lam].append(_timed(lambda: step(lam, cur, nxt)))
        torch.cuda.synchronize()
        tm.drain()
        for lam in (0.0, 1.0):
            r = _stats([a.elapsed_time(b) for a, b in sev[lam]])
            name = f"fit_step, lambda_pl = {lam:g} (8 + 8 scenes, fp16)"
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
