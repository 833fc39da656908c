"""GPU time of the pseudo-label kernels (csrc/pselab.hip) against what they replace.  Prints one JSON line per measurement.

(a) ``predict``: mm_pselab_predict against the sequence of torch ops that computes the same six tensors (two softmaxes, their
    average, three max-with-index, three casts to uint8), at the benchmark's point count per batch (8 scenes x 34,880 points).
(b) ``refine``: ``datasets.refine_pseudo_labels`` (numpy, one core, wall clock) against ``pselab.refine_pseudo_labels`` from host
    arrays to host arrays (upload, kernels, download; wall clock, synchronised) and its kernels alone (events), at 10^6, 10^7
    and 5 * 10^7 points with 6 and 11 classes.

GPU times by HIP events, medians of ``--reps`` after one warm-up; the host function is timed once per case above 10^6 points.

    python tools/bench_pselab.py [--reps 5] [--sizes 1000000 10000000 50000000] [--classes 6 11] [--skip-host-above N]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _events_ms(fn, reps):
    import torch

    times = []
    for r in range(reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        if r:
            times.append(ev[0].elapsed_time(ev[1]))
    return round(float(np.median(times)), 4)


def _torch_predict(a, b):
    import torch

    sa, sb = torch.softmax(a, 1), torch.softmax(b, 1)
    out = []
    for s in (sa, sb, 0.5 * (sa + sb)):
        p, i = s.max(1)
        out += [p, i.to(torch.uint8)]
    return out


def bench_predict(dev, reps, n, classes):
    import torch

    from mm2d3d_amd import pselab

    for C in classes:
        g = torch.Generator().manual_seed(C)
        a, b = (3 * torch.randn(n, C, generator=g)).to(dev), (3 * torch.randn(n, C, generator=g)).to(dev)
        res = {"what": "predict", "points": n, "classes": C, "hip_ms": _events_ms(lambda: pselab.predict(a, b), reps),
               "torch_ops_ms": _events_ms(lambda: _torch_predict(a, b), reps)}
        res["bytes_moved"] = n * (2 * C * 4 + 3 * 5)
        res["hip_gb_per_s"] = round(res["bytes_moved"] / res["hip_ms"] / 1e6, 1)
        print(json.dumps(res), flush=True)


def bench_refine(dev, reps, sizes, classes, skip_host_above):
    import torch

    from mm2d3d_amd import _lib, datasets, pselab

    L = _lib.lib()
    for n in sizes:
        for C in classes:
            rng = np.random.default_rng(n % 1000 + C)
            probs, labels = rng.random(n).astype(np.float32), rng.integers(0, C, n)
            res = {"what": "refine", "points": n, "classes": C}
            got = None
            wall = []
            for r in range(reps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = pselab.refine_pseudo_labels(probs, labels, num_classes=C, device=dev)
                torch.cuda.synchronize()
                if r:
                    wall.append((time.perf_counter() - t0) * 1e3)
            res["gpu_host_to_host_ms"] = round(float(np.median(wall)), 2)
            pd, yd = torch.from_numpy(probs).to(dev), torch.from_numpy(labels).to(dev)
            od = torch.empty_like(yd)
            ws = torch.empty(int(L.mm_pselab_refine_ws_bytes(C)), dtype=torch.uint8, device=dev)
            run = lambda: _lib.check(L.mm_pselab_refine(pd.data_ptr(), yd.data_ptr(), n, C, -100, od.data_ptr(), ws.data_ptr(), ws.numel(),
                                                        torch.cuda.current_stream().cuda_stream), "pselab_refine")
            res["gpu_kernels_ms"] = _events_ms(run, reps)
            del pd, yd, od
            if n <= skip_host_above:
                host = []
                for r in range(reps if n <= 1_000_000 else 1):
                    t0 = time.perf_counter()
                    want = datasets.refine_pseudo_labels(probs, labels)
                    host.append((time.perf_counter() - t0) * 1e3)
                res["host_numpy_ms"] = round(float(np.median(host)), 2)
                res["equal"] = bool(np.array_equal(got, want))
            print(json.dumps(res), flush=True)


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=8 * 34880, help="points per batch of the prediction measurement")
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 10_000_000, 50_000_000])
    ap.add_argument("--classes", type=int, nargs="+", default=[6, 11])
    ap.add_argument("--skip-host-above", type=int, default=50_000_000, help="do not time the host function above this many points")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    bench_predict(dev, args.reps, args.points, args.classes)
    bench_refine(dev, args.reps, args.sizes, args.classes, args.skip_host_above)


if __name__ == "__main__":
    main()
