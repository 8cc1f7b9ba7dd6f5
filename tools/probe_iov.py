#!/usr/bin/env python3
"""The list (fi_ioc) forms against one launch per segment (dev probe, GPU box).
One process, the two forms alternating round by round, float32 SUM:

  a  writev, 1024 segments of 4 KiB     vs the loop of lfa_atomic_write_async
  b  writev, 256 segments of 64 KiB     vs the same loop
  c  writev, 64 segments of 4 MiB       vs the same loop
  d  writev, one segment of 256 MiB     vs lfa_atomic_write_async
  e  reduce_treev, 8 inputs, 256 segments of 64 KiB
                                        vs the loop of lfa_reduce_tree_async

Both forms are called through ctypes with every argument array built
beforehand, so a round times the C entry points and the GPU, K calls of a
form between one HIP event pair.  A call's segments lie 64 bytes apart in a
region of a 256 MiB buffer; successive calls take other regions and other
buffer sets (4 x 2 x 256 MiB for the binary form, 9 x 256 MiB for the tree),
so the bytes a call touches were last touched more than the MALL's 256 MiB
ago.  Run it under a time limit (timeout -k 10 600 python tools/probe_iov.py).
Prints one JSON object and writes it to --out (default
profiles/iov_combine.json): median us per call of each form and loop / list,
and PASS or FAIL for each condition the list forms are held to:

  a, b  the single launch is faster than the loop (loop / list > 1)
  d     within 3 % of lfa_atomic_write_async (list / loop <= 1.03)

The exit status is 1 when a condition of a case that ran fails.
--parent-liblfa-bytes and --headline-parent / --headline-this (GiB/s of plain
bench.py runs, parent build and this one alternated in one job) are recorded
beside the figures; the headline must stay inside the 82.0-84.4 % of 8 TB/s
the README documents run to run, which is checked too when given.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libfabric_amd import _native  # noqa: E402
from libfabric_amd.enums import DT, OP  # noqa: E402

BUF = 256 << 20
GAP = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=8, help="calls of a form per timing")
    ap.add_argument("--cases", default="a,b,c,d,e")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "iov_combine.json"))
    ap.add_argument("--parent-liblfa-bytes", type=int, default=None)
    ap.add_argument("--headline-parent", default="", help="GiB/s, comma separated")
    ap.add_argument("--headline-this", default="", help="GiB/s, comma separated")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lib = _native.lib()
    ioc = _native.lfa_ioc
    g = torch.Generator(device="cuda").manual_seed(1)
    stream = torch.cuda.current_stream().cuda_stream
    op, dt = int(OP.SUM), int(DT.FLOAT)

    def raw():
        # small finite floats: sums of thousands of rounds stay finite
        return torch.rand(BUF // 4, device="cuda", generator=g).view(torch.uint8)

    sets = [(raw(), raw()) for _ in range(4)]
    tin = None

    def carve(nseg, seg_bytes):
        """Regions of a buffer that each hold nseg segments GAP bytes apart
        (16-byte aligned starts; segments that fill the buffer lie back to
        back); the one 256 MiB segment is the buffer."""
        if nseg == 1:
            return [[0]]
        pitch = seg_bytes + GAP if nseg * (seg_bytes + GAP) <= BUF else seg_bytes
        per = nseg * pitch
        return [[r * per + i * pitch for i in range(nseg)] for r in range(min(BUF // per, 16))]

    def binary_case(nseg, seg_bytes):
        n = seg_bytes // 4
        variants = []
        for region in carve(nseg, seg_bytes):
            for d, s in sets:
                da, sa = (ioc * nseg)(), (ioc * nseg)()
                for i, off in enumerate(region):
                    da[i].addr, da[i].count = d.data_ptr() + off, n
                    sa[i].addr, sa[i].count = s.data_ptr() + off, n
                variants.append((da, sa, [(d.data_ptr() + off, s.data_ptr() + off)
                                          for off in region]))

        def listed(i):
            da, sa, _ = variants[i % len(variants)]
            return lib.lfa_atomic_writev_async(op, dt, da, sa, nseg, stream)

        def loop(i):
            rc = 0
            for d, s in variants[i % len(variants)][2]:
                rc |= lib.lfa_atomic_write_async(op, dt, d, s, n, stream)
            return rc
        return listed, loop, len(variants), 3 * nseg * seg_bytes

    def tree_case(nseg, seg_bytes, nsrc):
        nonlocal tin
        tin = tin or [raw() for _ in range(nsrc)]
        n = seg_bytes // 4
        variants = []
        for region in carve(nseg, seg_bytes):
            for d, _ in sets[:2]:
                da = (ioc * nseg)()
                flat = (ctypes.c_void_p * (nseg * nsrc))()
                rows = []
                for i, off in enumerate(region):
                    da[i].addr, da[i].count = d.data_ptr() + off, n
                    row = (ctypes.c_void_p * nsrc)(*[t.data_ptr() + off for t in tin])
                    for k in range(nsrc):
                        flat[i * nsrc + k] = row[k]
                    rows.append((d.data_ptr() + off, row))
                variants.append((da, flat, rows))

        def listed(i):
            da, flat, _ = variants[i % len(variants)]
            return lib.lfa_reduce_treev_async(op, dt, da, flat, nsrc, nseg, stream)

        def loop(i):
            rc = 0
            for d, row in variants[i % len(variants)][2]:
                rc |= lib.lfa_reduce_tree_async(op, dt, d, row, nsrc, n, stream)
            return rc
        return listed, loop, len(variants), (nsrc + 1) * nseg * seg_bytes

    shapes = {"a": ("writev", 1024, 4 << 10), "b": ("writev", 256, 64 << 10),
              "c": ("writev", 64, 4 << 20), "d": ("writev", 1, 256 << 20),
              "e": ("reduce_treev", 256, 64 << 10)}
    cases = []
    for name in a.cases.split(","):
        form, nseg, seg = shapes[name]
        fns = binary_case(nseg, seg) if form == "writev" else tree_case(nseg, seg, 8)
        cases.append((name, form, nseg, seg, *fns))

    def run(fn, k0):
        for i in range(a.calls):
            if fn(k0 + i):
                raise RuntimeError("launch failed")

    k = 0
    for _ in range(2):                       # clock prewarm, every kernel loaded
        for _, _, _, _, listed, loop, _, _ in cases:
            run(listed, k)
            run(loop, k)
            k += a.calls
    torch.cuda.synchronize()
    times = {(name, which): [] for name, *_ in cases for which in ("list", "loop")}
    for _ in range(a.rounds):
        for name, _, _, _, listed, loop, _, _ in cases:
            for which, fn in (("list", listed), ("loop", loop)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(fn, k)
                e1.record()
                torch.cuda.synchronize()
                times[(name, which)].append(e0.elapsed_time(e1) * 1e3 / a.calls)
            k += a.calls
    out = {"device": torch.cuda.get_device_name(0), "op": "SUM", "datatype": "FLOAT",
           "rounds": a.rounds, "calls_per_timing": a.calls,
           "liblfa_bytes": os.path.getsize(_native.lib_path("lfa")), "cases": {}}
    for name, form, nseg, seg, _, _, nvar, nbytes in cases:
        li, lo = times[(name, "list")], times[(name, "loop")]
        ml, mo = statistics.median(li), statistics.median(lo)
        out["cases"][name] = {
            "form": form, "segments": nseg, "segment_bytes": seg, "buffer_variants": nvar,
            "list_us": round(ml, 2), "list_min_us": round(min(li), 2),
            "list_max_us": round(max(li), 2),
            "loop_us": round(mo, 2), "loop_min_us": round(min(lo), 2),
            "loop_max_us": round(max(lo), 2),
            "loop_over_list": round(mo / ml, 3),
            "list_frac_of_8TBs": round(nbytes / (ml * 1e-6) / 8e12, 4)}
    if a.parent_liblfa_bytes:
        out["liblfa_bytes_parent"] = a.parent_liblfa_bytes
        out["liblfa_growth"] = round(out["liblfa_bytes"] / a.parent_liblfa_bytes - 1, 4)
    conds = {}
    for name in ("a", "b"):
        if name in out["cases"]:
            conds[f"{name}: list faster than loop"] = out["cases"][name]["loop_over_list"] > 1
    if "d" in out["cases"]:
        c = out["cases"]["d"]
        c["list_over_loop"] = round(c["list_us"] / c["loop_us"], 4)
        conds["d: within 3 % of lfa_atomic_write_async"] = c["list_us"] <= 1.03 * c["loop_us"]
    hp = [float(x) for x in a.headline_parent.split(",") if x]
    ht = [float(x) for x in a.headline_this.split(",") if x]
    if hp and ht:
        mp, mt = statistics.median(hp), statistics.median(ht)
        out["headline_gib_s"] = {"parent": hp, "this": ht, "parent_median": mp,
                                 "this_median": mt,
                                 "how": "plain bench.py, the two builds alternated in one job"}
        # the documented run-to-run spread, as a ratio between two runs
        conds["headline: unchanged within the 82.0-84.4 % spread"] = \
            82.0 / 84.4 <= mt / mp <= 84.4 / 82.0
    out["conditions"] = {k: "PASS" if v else "FAIL" for k, v in conds.items()}
    for k, v in out["conditions"].items():
        print(f"{v}  {k}", flush=True)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0 if all(conds.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
