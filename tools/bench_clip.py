"""GPU time of the gradient-clipping kernels (csrc/clip.hip) against the yardstick ``mm_grad_nonfinite`` (csrc/optim.hip), which
reads the same bytes, and of a whole clipped update against the unclipped one of the same optimiser.

Sizes: the two parameter arenas of the benchmark's trainer (46,229,010 and 2,689,830 elements; tools/bench_optim.py prints them).
HIP events around ``--launches`` back-to-back launches, median of ``--reps`` after a warm-up; the yardstick is timed beside
every kernel, alternating, in the same run.  GB/s = 4 bytes per element read (``mm_grad_clip_value``: read, plus the write of the
vectors it changes - its figure counts the read only) over that time; ``ratio`` = GB/s over the yardstick's.  The whole steps are
the loss-scaled forms GradScaler.step_all queues for one arena: unclipped = mm_grad_nonfinite + prepare + ``*_step_dev``; clipped =
mm_grad_sqnorm (raises the flag itself) + mm_clip_finalize + prepare + ``*_step_dev``.  One JSON line per measurement, then a
markdown table.

    python tools/bench_clip.py [--reps 5] [--launches 10] [--sizes N ...] [--out profiles/optim/bench_clip.md]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [46229010, 2689830]


def _events_ms(fn, reps, launches):
    import torch

    times = []
    for r in range(reps + 2):  # two warm-up rounds
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(launches):
            fn()
        ev[1].record()
        ev[1].synchronize()
        if r >= 2:
            times.append(ev[0].elapsed_time(ev[1]) / launches)
    return float(np.median(times))


def main():
    import torch

    from mm2d3d_amd import _lib
    from mm2d3d_amd._lib import check

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10, help="back-to-back launches per timed sample")
    ap.add_argument("--sizes", type=int, nargs="+", default=SIZES, help="elements per arena")
    ap.add_argument("--out", default=None, help="also write the markdown table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip: needs a GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    lines = ["| elements | what | ms | GB/s | ratio | yardstick ms (same run) |", "|---:|---|---:|---:|---:|---:|"]
    for n in args.sizes:
        gen = torch.Generator().manual_seed(n % 9973)
        p, g = (torch.randn(n, generator=gen).to(dev) for _ in range(2))
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        g.mul_(1024.0)  # as under a loss scale
        scale = torch.full((1,), 1024.0, device=dev)
        eff, norm = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
        flags, step = torch.zeros(16, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        k = int(L.mm_grad_sqnorm_ws_bytes(n)) // 8
        part = torch.zeros(k, dtype=torch.float64, device=dev)
        counts = np.array([k], dtype=np.int64)
        coef = torch.zeros(int(L.mm_optim_coef_bytes()), dtype=torch.uint8, device=dev)
        P, G, M, V = (t.data_ptr() for t in (p, g, m, v))

        yard = lambda: check(L.mm_grad_nonfinite(G, n, flags.data_ptr(), s), "nonfinite")
        sqn = lambda: check(L.mm_grad_sqnorm(G, n, part.data_ptr(), 0, flags.data_ptr(), s), "sqnorm")
        fin = lambda sc: check(L.mm_clip_finalize(part.data_ptr(), counts.ctypes.data, 1, scale.data_ptr(), 1.0, sc, norm.data_ptr(),
                                                  eff.data_ptr(), s), "finalize")
        val = lambda: check(L.mm_grad_clip_value(G, n, 1.0, scale.data_ptr(), 1.0, s), "clip_value")

        def adamw(scale_t):
            check(L.mm_adam_prepare(scale_t.data_ptr(), flags.data_ptr(), 16, step.data_ptr(), 1, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, 1.0,
                                    coef.data_ptr(), s), "adam_prepare")
            check(L.mm_adam_step_dev(P, G, M, V, None, n, 1, coef.data_ptr(), s), "adamw_dev")

        def sgd(scale_t):
            check(L.mm_sgd_prepare(scale_t.data_ptr(), flags.data_ptr(), 16, step.data_ptr(), 1, 1e-3, 0.0, 0.0, 0.0, 1.0,
                                   coef.data_ptr(), s), "sgd_prepare")
            check(L.mm_sgd_step_dev(P, G, None, n, 0, coef.data_ptr(), s), "sgd_dev")

        measures = [("mm_grad_sqnorm", sqn), ("mm_clip_finalize", lambda: fin(1.0)), ("mm_grad_clip_value (first launch clamps 32%, the rest find nothing to clamp)", val)]
        for name, upd in (("adamw", adamw), ("sgd", sgd)):
            measures.append((f"{name} step, unclipped", lambda upd=upd: (yard(), upd(scale))))
            measures.append((f"{name} step, clipped", lambda upd=upd: (sqn(), fin(1.0), upd(eff))))
        yards = []
        for name, fn in measures:
            yards.append(_events_ms(yard, args.reps, args.launches))
            ms = _events_ms(fn, args.reps, args.launches)
            gbs = 4 * n / ms / 1e6
            row = dict(n=n, what=name, ms=round(ms, 4), yard_ms=round(yards[-1], 4))
            if name.startswith("mm_grad"):
                row.update(gb_per_s=round(gbs, 1), ratio=round(yards[-1] / ms, 3))
            print(json.dumps(row), flush=True)
            lines.append(f"| {n} | {name} | {ms:.4f} | {row.get('gb_per_s', '')} | {row.get('ratio', '')} | {yards[-1]:.4f} |")
        y = float(np.median(yards))
        print(json.dumps(dict(n=n, what="mm_grad_nonfinite (yardstick)", ms=round(y, 4), gb_per_s=round(4 * n / y / 1e6, 1),
                              ms_min=round(min(yards), 4), ms_max=round(max(yards), 4))), flush=True)
        lines.append(f"| {n} | mm_grad_nonfinite (yardstick, median of {len(yards)}) | {y:.4f} | {4 * n / y / 1e6:.1f} | 1.0 | "
                     f"{min(yards):.4f} .. {max(yards):.4f} |")
        assert int(flags.sum()) == 0 and bool(torch.isfinite(norm).all()), "the benchmark's gradients are finite"
        del p, g, m, v, part
    table = "\n".join(lines)
    print(table, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
