"""GPU time of the flat optimiser update kernels (csrc/optim.hip) against their own ``adamw`` variant, the update of the headline step.

Sizes: the two parameter arenas of the benchmark's trainer (bench.build_trainer: Net2DSeg / Net3DSeg; printed).  Per variant:
the plain entry point on a 16-byte aligned range (vector instantiation), the loss-scaled form (``*_step_dev``: coefficients read
from the device) and the plain form on a range that starts one element in (scalar instantiation).  HIP events around ``--launches``
back-to-back launches, median of ``--reps`` after a warm-up; GB/s = 4 bytes x (p, g and state arrays read + p and state arrays
written) per element over that time.  ``ratio`` = GB/s of the aligned plain form over the yardstick's (``adamw``, timed beside every
variant in the same run, alternating).  torch's own
optimiser on one GPU tensor of the same size is timed for context.  One JSON line per measurement, then a markdown table.

    python tools/bench_optim.py [--reps 5] [--launches 10] [--sizes N ...] [--out table.md]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, entry point family, number of state arrays, which of (s0, s1, s2) are passed, torch class + kwargs for context
VARIANTS = [
    ("sgd", "sgd", (0, 0, 0), dict(nesterov=0), ("SGD", dict(lr=1e-3))),
    ("sgd momentum", "sgd", (1, 0, 0), dict(nesterov=0), ("SGD", dict(lr=1e-3, momentum=0.9))),
    ("sgd nesterov", "sgd", (1, 0, 0), dict(nesterov=1), ("SGD", dict(lr=1e-3, momentum=0.9, nesterov=True))),
    ("adam", "adam", (1, 1, 0), dict(decoupled=0), ("Adam", dict(lr=1e-3))),
    ("adam amsgrad", "adam", (1, 1, 1), dict(decoupled=0), ("Adam", dict(lr=1e-3, amsgrad=True))),
    ("adamw", "adam", (1, 1, 0), dict(decoupled=1), ("AdamW", dict(lr=1e-3))),
    ("adamw amsgrad", "adam", (1, 1, 1), dict(decoupled=1), ("AdamW", dict(lr=1e-3, amsgrad=True))),
    ("rmsprop", "rmsprop", (1, 0, 0), {}, ("RMSprop", dict(lr=1e-3))),
    ("rmsprop momentum", "rmsprop", (1, 0, 1), {}, ("RMSprop", dict(lr=1e-3, momentum=0.9))),
    ("rmsprop centered", "rmsprop", (1, 1, 0), {}, ("RMSprop", dict(lr=1e-3, centered=True))),
    ("rmsprop centered momentum", "rmsprop", (1, 1, 1), {}, ("RMSprop", dict(lr=1e-3, centered=True, momentum=0.9))),
]


def arena_sizes():
    """Trainable elements of the two networks bench.build_trainer builds (their flat arenas)."""
    import bench
    from mm2d3d_amd.net2d import Net2DSeg
    from mm2d3d_amd.net3d import Net3DSeg

    count = lambda net: sum(p.numel() for p in net.parameters() if p.requires_grad)
    return count(Net2DSeg(6, pretrained=True)), count(Net3DSeg(6, True, bench.NET3D_KW))


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


def _launchers(L, fam, use, kw, bufs, n, off, coef):
    """(plain, dev) launch closures of one variant on elements [off, off + n) of the buffers."""
    import torch

    from mm2d3d_amd._lib import check

    s = torch.cuda.current_stream().cuda_stream
    at = lambda t: t.data_ptr() + 4 * off
    p, g = at(bufs["p"]), at(bufs["g"])
    st = [at(bufs[f"s{i}"]) if u else None for i, u in enumerate(use)]
    one, zero, step = bufs["one"].data_ptr(), bufs["zero"].data_ptr(), bufs["step"].data_ptr()
    if fam == "sgd":
        mom = 0.9 if use[0] else 0.0
        plain = lambda: check(L.mm_sgd_step(p, g, st[0], n, 1e-3, mom, 0.0, 1e-4, kw["nesterov"], 2, 1.0, None, 0, s), "sgd")
        check(L.mm_sgd_prepare(one, zero, 1, step, 0, 1e-3, mom, 0.0, 1e-4, 1.0, coef.data_ptr(), s), "prep")
        dev = lambda: check(L.mm_sgd_step_dev(p, g, st[0], n, kw["nesterov"], coef.data_ptr(), s), "sgd_dev")
    elif fam == "adam":
        d = kw["decoupled"]
        plain = lambda: check(L.mm_adam_step(p, g, st[0], st[1], st[2], n, 1e-3, 0.9, 0.999, 1e-8, 1e-2, d, 10, 1.0, None, 0, s), "adam")
        check(L.mm_adam_prepare(one, zero, 1, step, 0, 1e-3, 0.9, 0.999, 1e-8, 1e-2, d, 1.0, coef.data_ptr(), s), "prep")
        dev = lambda: check(L.mm_adam_step_dev(p, g, st[0], st[1], st[2], n, d, coef.data_ptr(), s), "adam_dev")
    else:
        mom = 0.9 if use[2] else 0.0
        plain = lambda: check(L.mm_rmsprop_step(p, g, st[0], st[1], st[2], n, 1e-3, 0.99, 1e-8, 1e-4, mom, 1.0, None, 0, s), "rms")
        check(L.mm_rmsprop_prepare(one, zero, 1, step, 0, 1e-3, 0.99, 1e-8, 1e-4, mom, 1.0, coef.data_ptr(), s), "prep")
        dev = lambda: check(L.mm_rmsprop_step_dev(p, g, st[0], st[1], st[2], n, coef.data_ptr(), s), "rms_dev")
    return plain, dev


def main():
    import torch

    from mm2d3d_amd import _lib

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10, help="back-to-back launches per timed sample")
    ap.add_argument("--sizes", type=int, nargs="+", default=None, help="elements per arena (default: the benchmark trainer's two arenas)")
    ap.add_argument("--out", default=None, help="also write the markdown table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim: needs a GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    sizes = args.sizes
    if sizes is None:
        n2d, n3d = arena_sizes()
        print(json.dumps({"what": "arena sizes", "2d_net": n2d, "3d_net": n3d}), flush=True)
        sizes = [n2d, n3d]
    rows = []
    for n in sizes:
        g_ = torch.Generator().manual_seed(n % 9973)
        bufs = {k: torch.randn(n + 4, generator=g_).to(dev) for k in ("p", "g")}
        bufs.update({k: torch.rand(n + 4, generator=g_).to(dev) for k in ("s0", "s1", "s2")})
        bufs.update(one=torch.ones(1, device=dev), zero=torch.zeros(1, dtype=torch.int32, device=dev),
                    step=torch.full((1,), 9, dtype=torch.int64, device=dev))
        coef = torch.zeros(int(L.mm_optim_coef_bytes()), dtype=torch.uint8, device=dev)
        yard, _ = _launchers(L, "adam", (1, 1, 0), dict(decoupled=1), bufs, n, 0, coef)
        yard_ms = []
        for name, fam, use, kw, (tcls, tkw) in VARIANTS:
            yard_ms.append(_events_ms(yard, args.reps, args.launches))  # the yardstick beside every variant: same run, alternating
            plain, devf = _launchers(L, fam, use, kw, bufs, n, 0, coef)
            ms = _events_ms(plain, args.reps, args.launches)
            dev_ms = _events_ms(devf, args.reps, args.launches)
            scalar, _ = _launchers(L, fam, use, kw, bufs, n, 1, coef)
            scalar_ms = _events_ms(scalar, args.reps, args.launches)
            tp = torch.nn.Parameter(bufs["p"][:n].clone())
            tp.grad = bufs["g"][:n].clone()
            topt = getattr(torch.optim, tcls)([tp], **tkw)
            torch_ms = _events_ms(topt.step, args.reps, 2)
            del topt, tp
            bytes_ = 4 * (3 + 2 * sum(use)) * n
            rows.append(dict(what="update", n=n, variant=name, bytes_per_elem=4 * (3 + 2 * sum(use)), ms=round(ms, 4),
                             gb_per_s=round(bytes_ / ms / 1e6, 1), dev_ms=round(dev_ms, 4), unaligned_ms=round(scalar_ms, 4),
                             torch_ms=round(torch_ms, 4), adamw_ms=round(yard_ms[-1], 4)))
            print(json.dumps(rows[-1]), flush=True)
        y = float(np.median(yard_ms))
        ygb = 28 * n / y / 1e6
        print(json.dumps(dict(what="yardstick", n=n, variant="adamw", bytes_per_elem=28, ms=round(y, 4), gb_per_s=round(ygb, 1),
                              ms_min=round(min(yard_ms), 4), ms_max=round(max(yard_ms), 4))), flush=True)
        for r in rows:
            if r["n"] == n:
                r["ratio"] = round(r["gb_per_s"] / ygb, 3)
        rows.append(dict(n=n, variant="adamw (yardstick)", bytes_per_elem=28, ms=round(y, 4), gb_per_s=round(ygb, 1), ratio=1.0))
        del bufs
    lines = ["| elements | variant | B/elem | ms | GB/s | ratio to adamw | *_step_dev ms | unaligned ms | torch.optim ms |",
             "|---:|---|---:|---:|---:|---:|---:|---:|---:|"]
    for r in rows:
        lines.append(f"| {r['n']} | {r['variant']} | {r['bytes_per_elem']} | {r['ms']:.4f} | {r['gb_per_s']:.0f} | {r['ratio']:.2f} | "
                     f"{r.get('dev_ms', '')} | {r.get('unaligned_ms', '')} | {r.get('torch_ms', '')} |")
    table = "\n".join(lines)
    print(table, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
