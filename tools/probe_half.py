#!/usr/bin/env python3
"""16-bit float combines against the float32 ones that move the same bytes
(dev probe, GPU box).  One process, interleaved rounds:

  combine   lfa_atomic_write_async at 256 MiB per operand: float SUM (the
            yardstick), bf16 SUM, fp16 SUM, bf16 MIN
  tree      lfa_reduce_tree_async, 8 inputs of 64 MiB: float SUM, bf16 SUM

K launches between one HIP event pair, buffer sets rotated past the MALL
(4 x 512 MiB for the combine, 2 x 576 MiB for the tree), a clock prewarm
first.  The operands are the same raw bytes for every type (the kernels have
no data-dependent path).  Prints one JSON object and writes it to --out
(default profiles/half_combine.json): median us per launch, the fraction of
8 TB/s the algorithmic bytes reach, and each 16-bit time over the float32
time of the same run.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libfabric_amd import atomic  # noqa: E402
from libfabric_amd.enums import DT, OP  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256, help="MiB per combine operand")
    ap.add_argument("--tree-mib", type=int, default=64, help="MiB per tree input")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "half_combine.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    S, T = a.mib << 20, a.tree_mib << 20
    g = torch.Generator(device="cuda").manual_seed(1)

    def raw(nbytes):
        return torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=g)

    sets = [(raw(S), raw(S)) for _ in range(4)]
    tsets = [([raw(T) for _ in range(8)], raw(T)) for _ in range(2)]

    def combine(dt, op):
        esz = atomic.reduce_datatype_size(dt)
        return lambda i: atomic.write(op, dt, sets[i % 4][0], sets[i % 4][1], S // esz)

    def tree(dt, op):
        esz = atomic.reduce_datatype_size(dt)
        return lambda i: atomic.reduce_tree(op, dt, tsets[i % 2][1], tsets[i % 2][0], T // esz)

    cases = [("combine_f32_sum", combine(DT.FLOAT, OP.SUM), 3 * S, None),
             ("combine_bf16_sum", combine(DT.BFLOAT16, OP.SUM), 3 * S, "combine_f32_sum"),
             ("combine_fp16_sum", combine(DT.FLOAT16, OP.SUM), 3 * S, "combine_f32_sum"),
             ("combine_bf16_min", combine(DT.BFLOAT16, OP.MIN), 3 * S, "combine_f32_sum"),
             ("tree8_f32_sum", tree(DT.FLOAT, OP.SUM), 9 * T, None),
             ("tree8_bf16_sum", tree(DT.BFLOAT16, OP.SUM), 9 * T, "tree8_f32_sum")]
    for _ in range(3):                       # clock prewarm, every kernel loaded
        for _, fn, _, _ in cases:
            for i in range(a.launches):
                fn(i)
    torch.cuda.synchronize()
    times = {name: [] for name, *_ in cases}
    for _ in range(a.rounds):
        for name, fn, _, _ in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.launches):
                fn(i)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / a.launches)
    out = {"device": torch.cuda.get_device_name(0), "mib_per_operand": a.mib,
           "tree_mib_per_input": a.tree_mib, "rounds": a.rounds, "launches": a.launches,
           "cases": {}}
    med = {name: statistics.median(ts) for name, ts in times.items()}
    for name, _, nbytes, base in cases:
        row = {"us": round(med[name], 2), "min_us": round(min(times[name]), 2),
               "max_us": round(max(times[name]), 2),
               "frac_of_8TBs": round(nbytes / (med[name] * 1e-6) / 8e12, 4)}
        if base:
            row["ratio_to_" + base] = round(med[name] / med[base], 4)
        out["cases"][name] = row
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
