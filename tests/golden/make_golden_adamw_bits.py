"""Bit-identity fixture of the AdamW update without ``amsgrad``: ``adamw_bits.npz``.

What it pins: the bits of FlatAdamW's update without ``amsgrad`` as an MI355X gave them at commit 93edc00, where csrc/loss.hip
had a kernel of its own for it; csrc/optim.hip k_optim (Adam with decoupled decay) is held to the same bits.  The fixture is this
project's own output; running the script again records whatever the current tree computes.
Only ``FlatAdamW``, ``GradScaler`` and a seeded CPU generator are used: the script runs unchanged on either side of that change,
and tests/test_gpu_optimizers.py imports ``run`` from here to repeat the runs.

Four runs = {plain, loss-scaled (init_scale 1024)} x {every parameter touched, parameter 0 never touched}; 4 steps each:

* every parameter touched: the range is the whole arena, 1047 elements from the 16-byte aligned base = one block of 1024 + a
  block whose sixth thread owns 3 elements (vector instantiation with a scalar tail);
* parameter 0 never touched: the range starts at offset 6 (not 16-byte aligned, scalar instantiation), 1041 elements = one
  block + 17, a one-element tail.

``p``, ``m``, ``v`` are stored as fp32 after step 1 (first-step bias corrections) and after step 4.

    python tests/golden/make_golden_adamw_bits.py [out.npz]
"""
import os
import sys

import numpy as np
import torch

SHAPES = [(6,), (1037,), (3, 1), (1,)]
N = 1047
HP = dict(lr=0.01, weight_decay=0.05, betas=(0.9, 0.999))
STEPS, STORED = 4, (1, 4)
# (key, loss-scaled, index of the first parameter that receives gradients, expected touched ranges)
RUNS = [
    ("plain_all", False, 0, [[0, 1047]]),
    ("plain_from6", False, 1, [[6, 1047]]),
    ("scaled_all", True, 0, [[0, 1047]]),
    ("scaled_from6", True, 1, [[6, 1047]]),
]


def run(dev, scaled, first):
    """-> ({"step<k>_<p|m|v>": fp32 CPU tensor}, [(touched ranges, data_ptr of the range start & 15) of every step])."""
    from mm2d3d_amd.amp import GradScaler
    from mm2d3d_amd.optimizers import FlatAdamW

    g = torch.Generator().manual_seed(29)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in SHAPES]
    o = FlatAdamW(ps, **HP)
    scaler = GradScaler(dev, init_scale=1024.0) if scaled else None
    out, seen = {}, []
    for step in range(1, STEPS + 1):
        ws = [torch.randn(s, generator=g) for s in SHAPES]
        o.zero_grad()
        loss = sum((p * w.to(dev)).sum() for p, w in zip(ps[first:], ws[first:]))
        (scaler.scale(loss) if scaled else loss).backward()
        a = o._arenas[0]
        ranges = o._touched_ranges(a)
        seen.append((ranges, a["p"][ranges[0][0]:].data_ptr() & 15))
        if scaled:
            scaler.step(o)
            scaler.update()
        else:
            o.step()
        if step in STORED:
            for name in ("p", "m", "v"):
                out[f"step{step}_{name}"] = a[name].detach().cpu().clone()
    return out, seen


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(os.path.dirname(here)))
    import mm2d3d_amd  # noqa: F401

    dev = torch.device("cuda:0")
    arrays = {}
    for key, scaled, first, ranges in RUNS:
        out, seen = run(dev, scaled, first)
        assert all(r == ranges for r, _ in seen), (key, seen)
        assert all((al == 0) == (first == 0) for _, al in seen), (key, seen)
        for k, t in out.items():
            assert t.dtype == torch.float32 and t.numel() == N and bool(torch.isfinite(t).all()), (key, k)
            arrays[f"{key}_{k}"] = t.numpy()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "adamw_bits.npz")
    np.savez(path, **arrays)
    print(f"wrote {path}: {len(arrays)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
