"""GPU time of the Lovasz-softmax loss of one segmentation head.

Shape: one head's source rows of the benchmark workload, N = 279,040, at C = 6 and C = 11; 3 * randn logits, labels with 5 %
ignored.

  A  ``losses.lovasz_softmax``: the segmented radix sort of csrc/lovasz.hip between two row kernels, one backward launch.
  B  the same loss composed from torch ops, written here: ``softmax``, per class ``torch.sort``, ``cumsum`` and the difference of
     the Jaccard loss (the paper's implementation), autograd assembling the gradient.

Forward plus backward, HIP events around every iteration, A and B alternating in one process after a warm-up of both; median,
10th / 90th percentile and minimum over ``--iters`` (>= 200) iterations each.  One JSON line per measurement, then a markdown table.

    python tools/bench_lovasz.py [--iters 200] [--out profiles/lovasz/bench_lovasz.md]

A's launch count comes from a kernel trace taken in a run of its own (tracing slows the host), of A alone:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_lovasz.py --only A --iters 20 --classes 6

dispatches of that run, less those of the same run with ``--iters 0``, over 20 (no GPU needed for the sum):

    python tools/bench_lovasz.py --count <dir> [--base <dir of the --iters 0 run>] --iters 20
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_ROWS = 279040


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

    def total_ns(d):
        out = {}
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True) if d else []:
            for r in csv.DictReader(open(f)):
                out[r["Name"]] = out.get(r["Name"], 0) + int(float(r["TotalDurationNs"]))
        return out

    run, base = calls(trace_dir), calls(base_dir)
    if not run:
        raise SystemExit(f"bench_lovasz: no *kernel_stats.csv under {trace_dir}")
    per = {k: (v - base.get(k, 0)) / iters for k, v in run.items() if v != base.get(k, 0)}
    ns, ns0 = total_ns(trace_dir), total_ns(base_dir)
    us = {k: round((ns[k] - ns0.get(k, 0)) / iters / 1e3, 2) for k in per}
    print(json.dumps(dict(launches_per_iteration=round(sum(per.values()), 2), kernels=per, kernel_us_per_iteration=us), indent=1))


def _timed(fn):
    import torch

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    return ev


def composite(x, y, classes="present", ignore_index=-100):
    """The loss from torch ops.  The Jaccard increments depend on the labels and the order only: constants of the gradient."""
    import torch

    C = x.shape[1]
    live = (y != ignore_index) & (y >= 0) & (y < C)
    p, y = torch.softmax(x.float(), 1)[live], y[live]
    if p.shape[0] == 0:
        return x.sum() * 0.0
    losses = []
    for c in range(C):
        fg = (y == c).float()
        if classes == "present" and fg.sum() == 0:
            continue
        es, order = torch.sort((fg - p[:, c]).abs(), dim=0, descending=True, stable=True)
        fs = fg[order]
        inter = fs.sum() - fs.cumsum(0)
        union = fs.sum() + (1 - fs).cumsum(0)
        jac = 1 - inter / union
        jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        losses.append(torch.dot(es, jac))
    return torch.stack(losses).mean()


def main():
    import torch

    from mm2d3d_amd.losses import lovasz_softmax

    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="timed iterations of A and of B")
    ap.add_argument("--rows", type=int, default=N_ROWS)
    ap.add_argument("--classes", type=int, nargs="+", default=[6, 11])
    ap.add_argument("--only", choices=["A", "B"], default=None, help="run --iters iterations of one variant alone (for a kernel trace)")
    ap.add_argument("--count", metavar="DIR", default=None, help="sum the kernel trace under DIR into launches per iteration")
    ap.add_argument("--base", metavar="DIR", default=None, help="with --count: the trace of the same run with --iters 0")
    ap.add_argument("--out", default=None, help="also write the markdown table to this file")
    args = ap.parse_args()
    if args.count:
        return _count(args.count, args.base, max(args.iters, 1))
    if not torch.cuda.is_available():
        raise SystemExit("bench_lovasz: needs a GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    N = args.rows
    lines = ["| what | median ms | p10 | p90 | min | n |", "|---|---:|---:|---:|---:|---:|"]
    for C in args.classes:
        gen = torch.Generator().manual_seed(5 + C)
        x = (3 * torch.randn(N, C, generator=gen)).to(dev).requires_grad_(True)
        y = torch.randint(0, C, (N,), generator=gen)
        y[torch.rand(N, generator=gen) < 0.05] = -100
        y = y.to(dev)

        def run_a():
            x.grad = None
            loss = lovasz_softmax(x, y)
            loss.backward()
            return loss

        def run_b():
            x.grad = None
            loss = composite(x, y)
            loss.backward()
            return loss

        if args.only:
            fn = run_a if args.only == "A" else run_b
            for _ in range(args.iters):
                fn()
            torch.cuda.synchronize()
            print(json.dumps(dict(what=f"{args.only} alone", iters=args.iters, N=N, C=C)))
            continue

        # the loss does not depend on the order of tied errors, single gradient entries do (a near tie may be ordered differently by
        # the two softmax evaluations): the losses must agree, the gradients are compared by their norm
        la, ga = run_a().item(), x.grad.clone()
        lb, gb = run_b().item(), x.grad.clone()
        diff = dict(loss=abs(la - lb), grad_rel_l2=((ga - gb).norm() / gb.norm()).item())
        print(json.dumps(dict(what="A against B", N=N, C=C, loss_a=la, loss_b=lb, **diff)), flush=True)
        assert diff["loss"] < 1e-4 and diff["grad_rel_l2"] < 1e-2, diff
        for _ in range(20):
            run_a(), run_b()
        torch.cuda.synchronize()
        evs = {"A": [], "B": []}
        for _ in range(max(args.iters, 1)):
            evs["A"].append(_timed(run_a))
            evs["B"].append(_timed(run_b))
        torch.cuda.synchronize()
        for k, name in (("A", "A lovasz_softmax, forward + backward"), ("B", "B torch composite (softmax, sort, cumsum), forward + backward")):
            r = _stats([a.elapsed_time(b) for a, b in evs[k]])
            print(json.dumps(dict(what=name, N=N, C=C, **r)), flush=True)
            lines.append("| {} (N = {}, C = {}) | {median_ms} | {p10_ms} | {p90_ms} | {min_ms} | {n} |".format(name, N, C, **r))
    if args.only:
        return
    table = "\n".join(lines)
    print(table, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
