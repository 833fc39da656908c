"""Adversarial output alignment against the same arithmetic composed from torch ops, HIP events, one GPU.

One head's rows of the benchmark workload (8 + 8 scenes, 558,080 point rows, 279,040 of them source), C = 6, H = 64:
  A  ``losses.adversarial`` forward + backward + the discriminator's ``FlatAdam`` step: three forward launches, one backward
     launch, one optimiser launch.
  B  the same arithmetic from torch ops: softmax or self-information, three ``F.linear`` with ``leaky_relu``, binary cross
     entropy with logits twice (on detached inputs for D; through D with frozen weights for the generator), autograd, then the
     same ``FlatAdam`` step.
A and B alternate after a warm-up of both.  Then ``fit_step`` on those batches with ``lambda_adv`` 0 against 0.001, alternating on
one trainer.  Prints one JSON line per measurement and a markdown table.

    python tools/bench_adversarial.py [--iters 200] [--steps 30] [--out profiles/adversarial/bench_adversarial.md]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("selfinfo", "softmax")
ON = 0.001  # lambda_adv of the "on" side of the step timing (AdvEnt's weight)


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

    from mm2d3d_amd.adversarial import initial_parameters
    from mm2d3d_amd.losses import adversarial
    from mm2d3d_amd.optimizers import FlatAdam
    from mm2d3d_amd.synthetic import make_batch

    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="timed iterations of each side in each mode")
    ap.add_argument("--steps", type=int, default=30, help="timed fit_step calls per side (0: skip the step timing)")
    ap.add_argument("--scenes", type=int, default=8, help="scenes per domain")
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--out", default=None, help="also write the markdown table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adversarial: needs a GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    B, C, H = args.scenes, 6, args.hidden
    mk = lambda j: {"source": make_batch(2, B, "nuscenes", (302, 480), 6, device=dev, augment=True, first_scene=j * B),
                    "target": make_batch(3, B, "nuscenes", (302, 480), 6, device=dev, augment=True, first_scene=j * B)}
    first = mk(0)
    P = int(first["source"]["x"][0].shape[0])
    N = P + int(first["target"]["x"][0].shape[0])
    gen = torch.Generator().manual_seed(5)
    x0 = 3 * torch.randn(N, C, generator=gen)
    x0[P:] = 1.5 * x0[P:] + 0.5
    x = x0.to(dev).requires_grad_(True)
    cut = np.cumsum([0, H * C, H, H * H, H, H, 1])

    def make_d():
        p = torch.nn.Parameter(initial_parameters(C, H, torch.Generator().manual_seed(0)).to(dev))
        return p, FlatAdam([p], lr=1e-4, betas=(0.9, 0.99))

    def step_d(opt, grad):
        opt.grad_arenas()[0].copy_(grad)
        opt.mark_all_touched()
        opt.step()

    def run_hip(p, opt, mode):
        x.grad = None
        out = adversarial(x, P, p.data, mode, H)
        step_d(opt, out["grad_params"])
        out["loss_g"].backward()
        return out["loss_g"], out["loss_d"]

    def run_torch(p, opt, mode):
        x.grad = None
        W1, b1, W2, b2, w3, b3 = (p[cut[i]:cut[i + 1]] for i in range(6))

        def disc(u, W1, b1, W2, b2, w3, b3):
            h = F.leaky_relu(F.linear(u, W1.view(H, C), b1), 0.2)
            h = F.leaky_relu(F.linear(h, W2.view(H, H), b2), 0.2)
            return F.linear(h, w3.view(1, H), b3).reshape(-1)

        prob = torch.softmax(x, dim=1)
        u = prob if mode == "softmax" else -prob * torch.log_softmax(x, dim=1) / math.log(C)
        a = disc(u.detach(), W1, b1, W2, b2, w3, b3)  # D's loss: the inputs are constants
        loss_d = 0.5 * F.binary_cross_entropy_with_logits(a[:P], torch.zeros_like(a[:P])) + \
            0.5 * F.binary_cross_entropy_with_logits(a[P:], torch.ones_like(a[P:]))
        (grad,) = torch.autograd.grad(loss_d, p)
        ag = disc(u[P:], *(t.detach() for t in (W1, b1, W2, b2, w3, b3)))  # the generator's: through D with frozen weights
        loss_g = F.binary_cross_entropy_with_logits(ag, torch.zeros_like(ag))
        step_d(opt, grad)
        loss_g.backward()
        return loss_g, loss_d

    sides = {"hip": run_hip, "torch": run_torch}
    lines = ["| what | median ms | p10 | p90 | min | n |", "|---|---:|---:|---:|---:|---:|"]
    for mode in MODES:
        state = {k: make_d() for k in sides}
        for _ in range(10):
            for k, fn in sides.items():
                fn(*state[k], mode)
        torch.cuda.synchronize()
        evs = {k: [] for k in sides}
        for _ in range(max(args.iters, 1)):
            for k, fn in sides.items():
                evs[k].append(_timed(lambda: fn(*state[k], mode)))
        torch.cuda.synchronize()
        for k, fn in sides.items():
            r = _stats([a.elapsed_time(b) for a, b in evs[k]])
            lg, ld = fn(*state[k], mode)
            what = "losses.adversarial" if k == "hip" else "torch ops + autograd"
            name = f"{what}, input {mode}, C = {C}, H = {H}: forward + backward + FlatAdam step of D"
            print(json.dumps(dict(what=name, N=N, P=P, loss_g=float(lg), loss_d=float(ld), **r)), flush=True)
            lines.append("| {} (N = {}, P = {}) | {median_ms} | {p10_ms} | {p90_ms} | {min_ms} | {n} |".format(name, N, P, **r))
        del state
    del x

    if args.steps > 0:
        import bench

        tm = bench.build_trainer(dev, train_kwargs={"precision": "fp16", "lambda_adv": ON, "adv_hidden": H})
        batches = [first] + [mk(j) for j in range(1, 4)]
        seq = [0]

        def next_batch():
            seq[0] += 1
            return bench.fresh(batches[(seq[0] - 1) % len(batches)])

        def step(on, cur, nxt):
            tm.lambda_adv = ON if on else 0.0  # read once per step by _generic_step: the same trainer and weights serve both sides
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
            name = f"fit_step, lambda_adv = {ON if on else 0:g} (8 + 8 scenes, fp16, input selfinfo, H = {H})"
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
