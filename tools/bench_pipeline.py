"""Training from files: the step time of ``fit_step`` when its batches come from the loaders, three ways, in one process.

    P   ``fit_step`` on four pre-built batches that live on the device and rotate (what bench.py times): the yardstick
    S   ``gpu_batch`` then ``fit_step(batch, next_batch=)``, one after the other on the host: what a user could do before
        mm2d3d_amd/pipeline.py (every ``gpu_batch`` waits for the step queued before it, several times)
    A   ``pipeline.BatchStream``: host phases on a worker thread, ``depth`` batches queued ahead, no host wait

Datasets: the full-size ones of tools/bench_imageprep.py (``make_dataset``), the same kind as source and as target, 8 + 8 scenes
per step (bench.py's default workload), ``image="gpu"``; the trainer is ``bench.build_trainer`` with the dataset's class count.
VirtualKITTI is run with ``use_rgb=True`` (the benchmark trainer's 3D net takes three input channels).  The loops alternate in
blocks of ``--block`` steps after ``--warmup`` steps each; a block is timed with one event per step on the stream (so host waits
that leave the GPU idle count) and by the wall clock.  Per dataset one JSON line:

    {P,S,A}_ms_p10_p50_p90   event time per step;  {P,S,A}_wall_ms  wall clock per step over the blocks
    loader_gpu_ms            GPU ms of one step's two batches in loop A (events around uploads, kernels and read-back)
    host_phase_ms            worker-thread ms of one step's two host phases;  result_wait_ms: ms inside ``result()`` per step
    expected_A_max           P p50 + loader_gpu_ms + (P p90 - P p10): the bound for a dataset whose host phase fits in a step

    python tools/bench_pipeline.py [--kind nuscenes a2d2 vkitti] [--steps 30] [--warmup 5] [--block 10] [--depth 2]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def pct(v):
    v = sorted(v)
    return [round(v[int(q * (len(v) - 1))], 3) for q in (0.1, 0.5, 0.9)]


def main():
    import torch

    import bench
    import bench_imageprep
    from mm2d3d_amd import datasets, pipeline

    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", nargs="+", default=["nuscenes", "a2d2", "vkitti"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--decode-threads", type=int, default=4)
    ap.add_argument("--loops", nargs="+", default=["P", "S", "A"], choices=["P", "S", "A"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    kw_batch = dict(device=dev, image="gpu", decode_threads=a.decode_threads)

    for kind in a.kind:
        with tempfile.TemporaryDirectory() as root:
            cls, kw = bench_imageprep.make_dataset(root, kind)
            if kind == "vkitti":
                kw["use_rgb"] = True
            src, trg = getattr(datasets, cls)(**kw), getattr(datasets, cls)(**kw)
            ncls = len(src.class_names)
            tm = bench.build_trainer(dev, num_classes=ncls, class_weights=[1.0] * ncls)
            B = a.scenes
            counter = [0]

            def step_indices():
                k = counter[0]
                counter[0] += 1
                return {"source": (src, [(B * k + j) % len(src) for j in range(B)]),
                        "target": (trg, [(B * k + 3 + j) % len(trg) for j in range(B)])}

            def load(step):
                return {name: ds.gpu_batch(idx, **kw_batch) for name, (ds, idx) in step.items()}

            np.random.seed(0)
            torch.manual_seed(0)
            prebuilt = [load(step_indices()) for _ in range(4)]
            rot = [0]

            def next_prebuilt():
                rot[0] += 1
                return bench.fresh(prebuilt[(rot[0] - 1) % 4])

            stats = []

            def run(loop, n, timed):
                """``n`` steps of one loop; returns (event ms per step, wall ms per step)."""
                marks = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
                torch.cuda.synchronize()
                if loop == "P":
                    nxt = next_prebuilt()
                    t0 = time.perf_counter()
                    marks[0].record()
                    for i in range(n):
                        cur, nxt = nxt, next_prebuilt()
                        tm.fit_step(cur, next_batch=nxt)
                        marks[i + 1].record()
                elif loop == "S":
                    nxt = load(step_indices())
                    t0 = time.perf_counter()
                    marks[0].record()
                    for i in range(n):
                        cur, nxt = nxt, load(step_indices())
                        tm.fit_step(cur, next_batch=nxt)
                        marks[i + 1].record()
                else:
                    steps = [step_indices() for _ in range(n + 1)]  # the last one is only announced as next_batch
                    with pipeline.BatchStream(steps, depth=a.depth, timing=True, **kw_batch) as stream:
                        for i, (cur, nxt) in enumerate(stream):
                            if i == 0:
                                t0 = time.perf_counter()
                                marks[0].record()
                            if i == n:
                                break
                            tm.fit_step(cur, next_batch=nxt)
                            marks[i + 1].record()
                        if timed:
                            stats.extend(stream.stats[2:])  # the first two were resolved before the first step was queued
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) * 1e3 / n
                return [marks[i].elapsed_time(marks[i + 1]) for i in range(n)], wall

            for loop in a.loops:
                run(loop, a.warmup, False)
            ev, wall = {l: [] for l in a.loops}, {l: [] for l in a.loops}
            done = 0
            while done < a.steps:
                n = min(a.block, a.steps - done)
                for loop in a.loops:
                    e, w = run(loop, n, True)
                    ev[loop] += e
                    wall[loop].append(w)
                done += n
            res = {"kind": kind, "scenes_per_step": 2 * B, "steps": a.steps, "warmup": a.warmup, "block": a.block, "depth": a.depth,
                   "points_per_step": int(sum(b["x"][0].shape[0] for b in prebuilt[0].values()))}
            for loop in a.loops:
                res[f"{loop}_ms_p10_p50_p90"] = pct(ev[loop])
                res[f"{loop}_wall_ms"] = round(float(np.mean(wall[loop])), 3)
            if stats:
                for key, name in (("gpu_ms", "loader_gpu_ms"), ("host_ms", "host_phase_ms"), ("wait_ms", "result_wait_ms")):
                    res[name] = round(float(np.median([s[key] for s in stats])), 3)
                if "P" in a.loops:
                    p10, p50, p90 = res["P_ms_p10_p50_p90"]
                    res["expected_A_max"] = round(p50 + res["loader_gpu_ms"] + (p90 - p10), 3)
                    res["host_bound"] = bool(res["host_phase_ms"] > p50)
            print(json.dumps(res), flush=True)
            del tm, prebuilt
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
