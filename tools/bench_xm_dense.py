"""GPU time of the sparse-to-dense cross-modal matching: the window search, the backward of the matched lift, and the step with
and without ``xm_window``.

Shape: the benchmark workload - the joined batch of ``make_batch`` for 8 + 8 scenes (bench.py --workload c2: 16 images of
302 x 480 pixels, N = 558,080 points, P = 279,040, C = 6); the two dense maps are the halves of one NHWC [16, 302, 480, 12] fp32
buffer as the fused heads leave them, map and rows = 3 * randn (every window then holds 9 / 25 / 49 unrelated rows - the trained
maps are smooth, which changes the matches, not the work).

  (a) ``mm_xm_search`` through ``losses._window_search`` for r = 0, 1, 2, 3, both directions: two launches each.
  (b) the backward of the lifted aux map: ``lifting.lift`` (the scatter over the index's own sort) against ``lifting.lift_at`` at
      the r = 2 selection (the sort of the selected keys, then the same scatter) - the sort is the difference.

HIP events around every call, the variants alternating in one process after a warm-up of all; median, 10th / 90th percentile and
minimum over ``--iters`` iterations each.

  (c) ``fit_step`` on those batches with ``xm_window`` 0 against 2, alternating on one trainer.

One JSON line per measurement, then a markdown table.

    python tools/bench_xm_dense.py [--iters 200] [--steps 30] [--out profiles/xmdense/bench_xm_dense.md]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ON = 2  # xm_window of the "on" side of the step timing


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

    from mm2d3d_amd import lifting
    from mm2d3d_amd.losses import _window_search
    from mm2d3d_amd.synthetic import make_batch

    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="timed iterations of each variant")
    ap.add_argument("--steps", type=int, default=30, help="timed fit_step calls per side (0: skip the step timing)")
    ap.add_argument("--scenes", type=int, default=8, help="scenes per domain")
    ap.add_argument("--out", default=None, help="also write the markdown table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_xm_dense: needs a GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    B, C, H, W = args.scenes, 6, 302, 480
    mk = lambda j: {"source": make_batch(2, B, "nuscenes", (H, W), C, device=dev, augment=True, first_scene=j * B),
                    "target": make_batch(3, B, "nuscenes", (H, W), C, device=dev, augment=True, first_scene=j * B)}
    first = mk(0)
    P = int(first["source"]["x"][0].shape[0])
    N = P + int(first["target"]["x"][0].shape[0])
    index = lifting.PixelIndex(list(first["source"]["img_indices"]) + list(first["target"]["img_indices"]), H, W, dev)
    assert index.n == N
    gen = torch.Generator().manual_seed(5)
    joint = (3 * torch.randn(2 * B, H, W, 2 * C, generator=gen)).to(dev)
    maps = joint.permute(0, 3, 1, 2)
    seg_main, seg_avg = maps[:, :C], maps[:, C:]
    rows = (3 * torch.randn(N, C, generator=gen)).to(dev)
    counts = torch.empty((2, 4), dtype=torch.int64, device=dev)
    lines = ["| what | median ms | p10 | p90 | min | n |", "|---|---:|---:|---:|---:|---:|"]

    def report(name, ms, **extra):
        r = _stats(ms)
        print(json.dumps(dict(what=name, N=N, P=P, **extra, **r)), flush=True)
        lines.append("| {} | {median_ms} | {p10_ms} | {p90_ms} | {min_ms} | {n} |".format(name, **r))

    # (a) the search
    variants = [(r, d) for r in (0, 1, 2, 3) for d in (0, 1)]
    search = lambda r, d: _window_search(seg_avg if d == 0 else seg_main, index, rows, r, P, d, counts[d])
    for _ in range(10):
        for r, d in variants:
            search(r, d)
    torch.cuda.synchronize()
    evs = {v: [] for v in variants}
    for _ in range(max(args.iters, 1)):
        for v in variants:
            evs[v].append(_timed(lambda: search(*v)))
    torch.cuda.synchronize()
    for r, d in variants:
        search(r, d)
        moved = counts[d, :2].sum().item() / N
        report(f"mm_xm_search r = {r}, direction {d} ({(2 * r + 1) ** 2} candidates)", [a.elapsed_time(b) for a, b in evs[(r, d)]], moved=round(moved, 4))

    # (b) the backward of the lifted aux map: its own pixels against a selection
    sel, _ = search(ON, 0)
    w = torch.randn(N, C, generator=gen).to(dev)
    avg = seg_avg.detach().contiguous().requires_grad_()  # a map of its own: both sides allocate and clear their gradient map

    def backward(selected):
        out = lifting.lift_at(avg, index, sel) if selected else lifting.lift(avg, index)
        return _timed(lambda: torch.autograd.grad(out, avg, w))

    for _ in range(10):
        backward(False), backward(True)
    torch.cuda.synchronize()
    bev = {False: [], True: []}
    for _ in range(max(args.iters, 1)):
        for s in (False, True):
            bev[s].append(backward(s))
    torch.cuda.synchronize()
    report("lift backward: scatter at the points' own pixels", [a.elapsed_time(b) for a, b in bev[False]])
    report(f"lift_at backward: sort of the selected keys + scatter (r = {ON} selection)", [a.elapsed_time(b) for a, b in bev[True]])

    if args.steps > 0:
        import bench

        tm = bench.build_trainer(dev, train_kwargs={"precision": "fp16", "xm_window": ON})
        batches = [first] + [mk(j) for j in range(1, 4)]
        seq = [0]

        def next_batch():
            seq[0] += 1
            return bench.fresh(batches[(seq[0] - 1) % len(batches)])

        def step(on, cur, nxt):
            tm.xm_window = ON if on else 0  # read once per step by _generic_step: the same trainer and weights serve both sides
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
            report(f"fit_step, xm_window = {ON if on else 0} (8 + 8 scenes, fp16)", [a.elapsed_time(b) for a, b in sev[on]])
    table = "\n".join(lines)
    print(table, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
