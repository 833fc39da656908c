"""GPU time of the target-domain entropy and diversity terms of one head of the joined step, and of the step with and without them.

Shape: the rows of one head on the benchmark workload - the joined point count of ``make_batch`` for 8 + 8 scenes
(bench.py --workload c2: N = 558,080, P = 279,040), C = 6, logits 3 * randn; rows [0, P) are the source's, rows [P, N) the target's.

  A  ``losses.target_entropy``: two forward launches, one backward launch for both terms.
  B  the same two terms composed from torch ops on the row slice (``softmax``, ``log_softmax``, masked means over the rows whose
     logits are finite), autograd assembling the gradient of the whole tensor.

Forward plus backward of ``ent + div``, HIP events around every iteration, A and B alternating in one process after a warm-up of
both; median, 10th / 90th percentile and minimum over ``--iters`` (>= 200) iterations each.  Then ``fit_step`` on those batches
with both weights 0 against ``lambda_minent`` 0.3 / ``lambda_div`` 0.2, alternating on one trainer.  One JSON line per
measurement, then a markdown table.

    python tools/bench_infomax.py [--iters 200] [--steps 30] [--out profiles/infomax/bench_infomax.md]

Launch counts come from a kernel trace taken in a run of its own (tracing slows the host), of one variant alone:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bench_infomax.py --only A --iters 20

dispatches of that run, less those of the same run with ``--iters 0``, over 20 (tools/bench_pl_loss.py --count sums them).
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C = 6
PRIOR = [3.0, 1.0, 2.0, 1.0, 0.5, 2.5]
ON = (0.3, 0.2)  # lambda_minent, lambda_div of the "on" side of the step timing


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

    from mm2d3d_amd.losses import target_entropy
    from mm2d3d_amd.synthetic import make_batch

    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="timed iterations of A and of B")
    ap.add_argument("--steps", type=int, default=30, help="timed fit_step calls per side (0: skip the step timing)")
    ap.add_argument("--scenes", type=int, default=8, help="scenes per domain")
    ap.add_argument("--only", choices=["A", "B"], default=None, help="run --iters iterations of one variant alone (for a kernel trace)")
    ap.add_argument("--out", default=None, help="also write the markdown table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_infomax: needs a GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    B = args.scenes
    mk = lambda j: {"source": make_batch(2, B, "nuscenes", (302, 480), 6, device=dev, augment=True, first_scene=j * B),
                    "target": make_batch(3, B, "nuscenes", (302, 480), 6, device=dev, augment=True, first_scene=j * B)}
    first = mk(0)
    P = int(first["source"]["x"][0].shape[0])
    N = P + int(first["target"]["x"][0].shape[0])
    gen = torch.Generator().manual_seed(5)
    x = (3 * torch.randn(N, C, generator=gen)).to(dev).requires_grad_(True)
    pi = torch.tensor(PRIOR, dtype=torch.float64)
    log_pi = (pi / pi.sum()).log().to(torch.float32).to(dev)
    ln_c = math.log(C)

    def run_a():
        x.grad = None
        ent, div, _, _ = target_entropy(x, P, PRIOR)
        (ent + div).backward()
        return ent, div

    def run_b():
        x.grad = None
        t = x[P:]
        ok = torch.isfinite(t).all(1)
        n = ok.sum().clamp(min=1)
        p, lp = torch.softmax(t, 1), torch.log_softmax(t, 1)
        ent = torch.where(ok, -(p * lp).sum(1), 0.0).sum() / (n * ln_c)
        mass = torch.where(ok[:, None], p, 0.0).sum(0) / n
        div = (mass * (mass.log() - log_pi)).sum() / ln_c
        (ent + div).backward()
        return ent, div

    if args.only:
        fn = run_a if args.only == "A" else run_b
        for _ in range(args.iters):
            fn()
        torch.cuda.synchronize()
        print(json.dumps(dict(what=f"{args.only} alone", iters=args.iters, N=N, P=P)))
        return

    # faster and different is not faster: the two variants compute the same numbers (B sums in float32, in an order of its own)
    la, ga = [v.item() for v in run_a()], x.grad.clone()
    lb, gb = [v.item() for v in run_b()], x.grad.clone()
    diff = dict(ent=abs(la[0] - lb[0]), div=abs(la[1] - lb[1]), grad_max_abs_times_n=(ga - gb).abs().max().item() * (N - P))
    print(json.dumps(dict(what="A against B", N=N, P=P, **diff)), flush=True)
    assert diff["ent"] < 1e-4 and diff["div"] < 1e-4 and diff["grad_max_abs_times_n"] < 1e-4, diff
    for _ in range(20):
        run_a(), run_b()
    torch.cuda.synchronize()
    evs = {"A": [], "B": []}
    for _ in range(max(args.iters, 1)):
        evs["A"].append(_timed(run_a))
        evs["B"].append(_timed(run_b))
    torch.cuda.synchronize()
    lines = ["| what | median ms | p10 | p90 | min | n |", "|---|---:|---:|---:|---:|---:|"]
    for k, name in (("A", "A target_entropy, forward + backward"), ("B", "B softmax / log_softmax / masked means, forward + backward")):
        r = _stats([a.elapsed_time(b) for a, b in evs[k]])
        print(json.dumps(dict(what=name, N=N, P=P, C=C, **r)), flush=True)
        lines.append("| {} (N = {}, P = {}) | {median_ms} | {p10_ms} | {p90_ms} | {min_ms} | {n} |".format(name, N, P, **r))

    if args.steps > 0:
        import bench

        tm = bench.build_trainer(dev, train_kwargs={"precision": "fp16", "lambda_minent": ON[0], "lambda_div": ON[1], "div_prior": PRIOR})
        batches = [first] + [mk(j) for j in range(1, 4)]
        seq = [0]

        def next_batch():
            seq[0] += 1
            return bench.fresh(batches[(seq[0] - 1) % len(batches)])

        def step(on, cur, nxt):
            # read once per step by _generic_step: the same trainer and weights serve both sides
            tm.lambda_minent, tm.lambda_div = (ON if on else (0.0, 0.0))
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
            name = f"fit_step, lambda_minent = {ON[0] if on else 0:g}, lambda_div = {ON[1] if on else 0:g} (8 + 8 scenes, fp16)"
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
