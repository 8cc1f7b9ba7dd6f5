#!/usr/bin/env python3
"""The fetch and compare list (fi_ioc) forms against one launch per segment
(dev probe, GPU box), tools/probe_iov.py's protocol.  One process, the two
forms alternating round by round, float32 SUM readwrite and float32 CSWAP:

  a  1024 segments of 4 KiB      vs the loop of the contiguous call
  b  256 segments of 64 KiB      vs the same loop
  d  one segment of 256 MiB      vs the contiguous call

Both forms are called through ctypes with every argument array built
beforehand, so a round times the C entry points and the GPU, K calls of a
form between one HIP event pair.  A call's segments lie 64 bytes apart in a
region of a 256 MiB buffer; successive calls take other regions and other
buffer sets (3 x 4 x 256 MiB: dst, src, cmp, res), so the bytes a call touches
were last touched more than the MALL's 256 MiB ago.  Run it under a time limit
(timeout -k 10 600 python tools/probe_iov_fetch.py).  Prints one JSON object
and writes it to --out (default profiles/iov_fetch_combine.json): median us
per call of each form and loop / list, and PASS or FAIL for each condition the
list forms are held to:

  a, b  the single launch is faster than the loop (loop / list > 1)
  d     within 3 % of the contiguous call (list / loop <= 1.03)

The exit status is 1 when a condition of a case that ran fails.
--parent-liblfa-bytes and --headline-parent / --headline-this (GiB/s of plain
bench.py runs, parent build and this one alternated in one job) are recorded
beside the figures; the headline must stay inside the 82.0-84.4 % of 8 TB/s
the README documents run to run, which is checked too when given.
"""
import argparse
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
CSWAP = 12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=8, help="calls of a form per timing")
    ap.add_argument("--cases", default="a,b,d")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "iov_fetch_combine.json"))
    ap.add_argument("--parent-liblfa-bytes", type=int, default=None)
    ap.add_argument("--headline-parent", default="", help="GiB/s, comma separated")
    ap.add_argument("--headline-this", default="", help="GiB/s, comma separated")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lib = _native.lib()
    ioc = _native.lfa_ioc
    g = torch.Generator(device="cuda").manual_seed(1)
    stream = torch.cuda.current_stream().cuda_stream
    dt = int(DT.FLOAT)

    def raw():
        # small finite floats: sums of thousands of rounds stay finite
        return torch.rand(BUF // 4, device="cuda", generator=g).view(torch.uint8)

    sets = [tuple(raw() for _ in range(4)) for _ in range(3)]    # dst, src, cmp, res

    def carve(nseg, seg_bytes):
        if nseg == 1:
            return [[0]]
        pitch = seg_bytes + GAP if nseg * (seg_bytes + GAP) <= BUF else seg_bytes
        per = nseg * pitch
        return [[r * per + i * pitch for i in range(nseg)] for r in range(min(BUF // per, 16))]

    def case(compare, nseg, seg_bytes):
        n = seg_bytes // 4
        op = CSWAP if compare else int(OP.SUM)
        variants = []
        for region in carve(nseg, seg_bytes):
            for bufs in sets:
                use = bufs if compare else (bufs[0], bufs[1], bufs[3])
                arrs = [(ioc * nseg)() for _ in use]
                for arr, t in zip(arrs, use):
                    for i, off in enumerate(region):
                        arr[i].addr, arr[i].count = t.data_ptr() + off, n
                variants.append((arrs, [[t.data_ptr() + off for t in use] for off in region]))
        if compare:
            listfn, onefn = lib.lfa_atomic_swapv_async, lib.lfa_atomic_swap_async
        else:
            listfn, onefn = lib.lfa_atomic_readwritev_async, lib.lfa_atomic_readwrite_async

        def listed(i):
            return listfn(op, dt, *variants[i % len(variants)][0], nseg, stream)

        def loop(i):
            rc = 0
            for ptrs in variants[i % len(variants)][1]:
                rc |= onefn(op, dt, *ptrs, n, stream)
            return rc
        # bytes moved: every input read, res and dst written
        return listed, loop, len(variants), (5 if compare else 4) * nseg * seg_bytes

    shapes = {"a": (1024, 4 << 10), "b": (256, 64 << 10), "d": (1, 256 << 20)}
    cases = []
    for name in a.cases.split(","):
        nseg, seg = shapes[name]
        for compare in (False, True):
            form = "swapv CSWAP" if compare else "readwritev SUM"
            cases.append((name + (" cswap" if compare else " sum"), form, nseg, seg,
                          *case(compare, nseg, seg)))

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
    out = {"device": torch.cuda.get_device_name(0), "datatype": "FLOAT",
           "rounds": a.rounds, "calls_per_timing": a.calls,
           "liblfa_bytes": os.path.getsize(_native.lib_path("lfa")), "cases": {}}
    conds = {}
    for name, form, nseg, seg, _, _, nvar, nbytes in cases:
        li, lo = times[(name, "list")], times[(name, "loop")]
        ml, mo = statistics.median(li), statistics.median(lo)
        c = out["cases"][name] = {
            "form": form, "segments": nseg, "segment_bytes": seg, "buffer_variants": nvar,
            "list_us": round(ml, 2), "list_min_us": round(min(li), 2),
            "list_max_us": round(max(li), 2),
            "loop_us": round(mo, 2), "loop_min_us": round(min(lo), 2),
            "loop_max_us": round(max(lo), 2),
            "loop_over_list": round(mo / ml, 3),
            "list_frac_of_8TBs": round(nbytes / (ml * 1e-6) / 8e12, 4)}
        if name[0] in "ab":
            conds[f"{name}: list faster than loop"] = mo / ml > 1
        else:
            c["list_over_loop"] = round(ml / mo, 4)
            conds[f"{name}: within 3 % of the contiguous call"] = ml <= 1.03 * mo
    if a.parent_liblfa_bytes:
        out["liblfa_bytes_parent"] = a.parent_liblfa_bytes
        out["liblfa_growth"] = round(out["liblfa_bytes"] / a.parent_liblfa_bytes - 1, 4)
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
