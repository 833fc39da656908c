"""Launches per training step from kernel traces (``rocprofv3 --kernel-trace --stats``), by differencing.

A traced process also builds a trainer, warms up and captures graphs, so one run's totals say nothing about a step.  Two runs of the
same command that differ only in the number of steps (N1 < N2) do: (calls_2 - calls_1) / (N2 - N1) per kernel name, and the same
for the summed kernel durations.

    python tools/trace_counts.py NAME=stats_n1.csv,stats_n2.csv,N1,N2 [NAME=...] [--out launch_counts.json]

With the sides ``batch`` and ``teacher`` of tools/bench_teacher.py it also lists ``teacher_minus_batch``: the teacher pass.
"""
import argparse
import csv
import json


def column(path, name, kind):
    with open(path, newline="") as f:
        return {r["Name"]: kind(r[name]) for r in csv.DictReader(f)}


def per_step(p1, p2, n1, n2, name="Calls", kind=int, scale=1.0, digits=3):
    c1, c2 = column(p1, name, kind), column(p2, name, kind)
    out = {k: (c2.get(k, 0) - c1.get(k, 0)) * scale / (n2 - n1) for k in sorted(set(c1) | set(c2))}
    return {k: round(v, digits) for k, v in out.items() if round(v, digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sides", nargs="+")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {}
    for spec in args.sides:
        name, rest = spec.split("=", 1)
        p1, p2, n1, n2 = rest.split(",")
        k = per_step(p1, p2, int(n1), int(n2))
        ms = per_step(p1, p2, int(n1), int(n2), "TotalDurationNs", float, 1e-6, 4)  # summed kernel durations: no gaps, no overlap
        res[name] = {"steps_differenced": [int(n1), int(n2)], "launches_per_step": round(sum(k.values()), 2),
                     "kernel_ms_per_step": round(sum(ms.values()), 3), "kernels": k, "kernel_ms": ms}
    if "batch" in res and "teacher" in res:
        a, b = res["batch"]["kernels"], res["teacher"]["kernels"]
        d = {k: round(b.get(k, 0) - a.get(k, 0), 3) for k in sorted(set(a) | set(b))}
        d = {k: v for k, v in d.items() if v}
        ma, mb = res["batch"]["kernel_ms"], res["teacher"]["kernel_ms"]
        m = {k: round(mb.get(k, 0) - ma.get(k, 0), 4) for k in sorted(set(ma) | set(mb))}
        m = {k: v for k, v in m.items() if v}
        res["teacher_minus_batch"] = {"launches_per_step": round(sum(d.values()), 2), "kernel_ms_per_step": round(sum(m.values()), 3),
                                      "kernels": d, "kernel_ms": m}
    for name, r in res.items():
        print(name, r["launches_per_step"], "launches,", r["kernel_ms_per_step"], "ms of kernels per step")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
