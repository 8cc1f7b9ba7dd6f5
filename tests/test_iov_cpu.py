"""The list (fi_ioc) forms without a GPU: struct lfa_ioc's layout, the exported
symbols, lfa_host_writev against the loop of lfa_host_write, and every
argument error of the three entry points (all reported before anything is
touched or enqueued, so the device forms' errors need no GPU either)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from libfabric_amd import _native, atomic
from tests import _iov_layout as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/include"
EINVAL, EOPNOTSUPP = -22, -95
ioc = _native.lfa_ioc


def _aligned(a: np.ndarray) -> np.ndarray:
    """A copy of the byte array `a` whose first byte is 16-byte aligned."""
    raw = np.empty(a.size + 16, np.uint8)
    lead = -raw.ctypes.data % 16
    out = raw[lead:lead + a.size]
    out[:] = a
    return out


def _iocs(arena, segs, esz):
    arr = (ioc * max(len(segs), 1))()
    for i, (lo, nb) in enumerate(segs):
        arr[i].addr = arena.ctypes.data + lo
        arr[i].count = nb // esz
    return arr


def test_ioc_layout():
    assert ctypes.sizeof(ioc) == 16
    assert ioc.addr.offset == 0 and ioc.count.offset == 8
    assert atomic.LFA_IOV_MAX == 4096
    lines = ["#include <stddef.h>", '#include "lfa_fabric.h"',
             "#define EQ(a, b) _Static_assert((long long)(a) == (long long)(b), #a)",
             "EQ(sizeof(struct lfa_ioc), 16);", "EQ(offsetof(struct lfa_ioc, addr), 0);",
             "EQ(offsetof(struct lfa_ioc, count), 8);", "EQ(LFA_IOV_MAX, 4096);"]
    inc = ["-I", os.path.join(ROOT, "include")]
    if os.path.isdir(REF):      # the same static-assert compile as tests/test_abi.py
        lines.insert(1, "#include <rdma/fabric.h>")
        lines += ["EQ(sizeof(struct fi_ioc), sizeof(struct lfa_ioc));",
                  "EQ(offsetof(struct fi_ioc, addr), offsetof(struct lfa_ioc, addr));",
                  "EQ(offsetof(struct fi_ioc, count), offsetof(struct lfa_ioc, count));"]
        inc += ["-I", REF]
    lines.append("int main(void) { return 0; }")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "ioc.c")
        open(src, "w").write("\n".join(lines) + "\n")
        r = subprocess.run(["gcc", "-std=gnu11", *inc, "-c", src, "-o",
                            os.path.join(d, "ioc.o")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_symbols_exported():
    lib = _native.lib()
    for name in ("lfa_atomic_writev_async", "lfa_reduce_treev_async", "lfa_host_writev"):
        assert hasattr(lib, name), name


DTS = (L.INT8, L.BFLOAT16, L.FLOAT, L.DOUBLE, L.INT128, L.FLOAT_COMPLEX)
OPS = (L.SUM, L.MIN, L.PROD, L.LXOR, L.BXOR)


@pytest.mark.parametrize("dt", DTS)
def test_host_writev_equals_loop(dt):
    esz = L.ESZ[dt]
    ran = 0
    for op in OPS:
        if op == L.BXOR and dt not in L.INTEGERS:
            continue                # a bitwise op: integer datatypes only
        if atomic.reduce_valid(dt, op):
            continue                # MIN has no float complex handler
        counts, offsets, (segs, size) = L.standard(37, esz, shift=op)
        assert set(counts) == set(L.COUNTS) and set(offsets) == set(L.OFFSETS)
        d0 = _aligned(L.fill(size, segs, 100 + op, dt))
        s0 = _aligned(L.fill(size, segs, 200 + op, dt))
        for (lo, _), off in zip(segs, offsets):
            assert (d0.ctypes.data + lo) % 16 == off
        want, got, src = _aligned(d0), _aligned(d0), _aligned(s0)
        for lo, nb in segs:
            rc = _native.lib().lfa_host_write(op, dt, want.ctypes.data + lo,
                                              src.ctypes.data + lo, nb // esz)
            assert rc == 0
        rc = _native.lib().lfa_host_writev(op, dt, _iocs(got, segs, esz),
                                           _iocs(src, segs, esz), len(segs))
        assert rc == 0
        assert np.array_equal(got, want), (op, dt)
        assert not np.array_equal(got, d0)
        assert L.gaps_intact(got, segs) and np.array_equal(src, s0)
        ran += 1
    assert ran >= 3


def test_host_writev_python_form():
    d = [np.arange(n, dtype=np.float32) for n in (5, 0, 17)]
    s = [np.full(n, 2, np.float32) for n in (5, 0, 17)]
    atomic.host_writev(L.SUM, L.FLOAT, d, s)
    for n, x in zip((5, 0, 17), d):
        assert np.array_equal(x, np.arange(n, dtype=np.float32) + 2)
    with pytest.raises(atomic.LfaError) as e:
        atomic.host_writev(L.BXOR, L.FLOAT, d, s)
    assert e.value.rc == EOPNOTSUPP


def _error_cases(arena, src):
    """(name, dst list, src list, nseg, want) — bad calls on float32 segments."""
    base, sbase = arena.ctypes.data, src.ctypes.data

    def arr(items):
        a = (ioc * max(len(items), 1))()
        for i, (p, n) in enumerate(items):
            a[i].addr, a[i].count = p, n
        return a
    good_d = arr([(base + 64, 8), (base + 256, 8)])
    good_s = arr([(sbase + 64, 8), (sbase + 256, 8)])
    many = arr([(base + 64 + 4 * i, 1) for i in range(atomic.LFA_IOV_MAX + 1)])
    many_s = arr([(sbase + 64 + 4 * i, 1) for i in range(atomic.LFA_IOV_MAX + 1)])
    return [
        ("null dst array", None, good_s, 2, EINVAL),
        ("null src array", good_d, None, 2, EINVAL),
        ("null dst addr", arr([(None, 8), (base + 256, 8)]), good_s, 2, EINVAL),
        ("null src addr", good_d, arr([(sbase + 64, 8), (None, 8)]), 2, EINVAL),
        ("count mismatch", good_d, arr([(sbase + 64, 8), (sbase + 256, 7)]), 2, EINVAL),
        ("too many segments", many, many_s, atomic.LFA_IOV_MAX + 1, EINVAL),
        ("overlap", arr([(base + 64, 8), (base + 1024, 4), (base + 92, 8)]),
         arr([(sbase + 64, 8), (sbase + 1024, 4), (sbase + 512, 8)]), 3, EINVAL),
        ("contained", arr([(base + 64, 64), (base + 128, 4)]),
         arr([(sbase + 64, 64), (sbase + 1024, 4)]), 2, EINVAL),
    ]


@pytest.mark.parametrize("entry", ["lfa_host_writev", "lfa_atomic_writev_async"])
def test_writev_errors_leave_buffers_untouched(entry):
    lib = _native.lib()
    size = 64 + 4 * (atomic.LFA_IOV_MAX + 1) + 4096
    d0 = np.random.default_rng(1).integers(0, 256, size, dtype=np.uint8)
    s0 = np.random.default_rng(2).integers(0, 256, size, dtype=np.uint8)
    arena, src = _aligned(d0), _aligned(s0)
    fn = getattr(lib, entry)
    tail = (None,) if entry.endswith("async") else ()

    for name, d, s, nseg, want in _error_cases(arena, src):
        assert fn(L.SUM, L.FLOAT, d, s, nseg, *tail) == want, name
        assert np.array_equal(arena, d0) and np.array_equal(src, s0), name
    good = _error_cases(arena, src)[1][1]
    good_s = _error_cases(arena, src)[0][2]
    # unsupported pairs: bitwise on a float, MIN on float complex, a datatype
    # and an op outside the tables
    for op, dt in ((L.BXOR, L.FLOAT), (L.MIN, L.FLOAT_COMPLEX), (L.SUM, 12), (10, L.FLOAT),
                   (19, L.FLOAT)):
        assert fn(op, dt, good, good_s, 2, *tail) == EOPNOTSUPP, (op, dt)
    assert np.array_equal(arena, d0) and np.array_equal(src, s0)
    # nothing to do is not an error: no segments, or only empty ones
    assert fn(L.SUM, L.FLOAT, None, None, 0, *tail) == 0
    empty = (ioc * 2)()
    assert fn(L.SUM, L.FLOAT, empty, empty, 2, *tail) == 0
    # segments that touch without sharing a byte are fine (host form: it runs)
    if not tail:
        a = (ioc * 2)()
        b = (ioc * 2)()
        for i in range(2):
            a[i].addr, a[i].count = arena.ctypes.data + 64 + 32 * i, 8
            b[i].addr, b[i].count = src.ctypes.data + 64 + 32 * i, 8
        assert fn(L.SUM, L.FLOAT, a, b, 2) == 0
        assert not np.array_equal(arena, d0)


def test_treev_errors():
    lib = _native.lib()
    d0 = np.random.default_rng(3).integers(0, 256, 4096, dtype=np.uint8)
    arena = _aligned(d0)
    base = arena.ctypes.data

    def arr(items):
        a = (ioc * len(items))()
        for i, (p, n) in enumerate(items):
            a[i].addr, a[i].count = p, n
        return a
    dst = arr([(base + 64, 8), (base + 256, 8)])
    srcs = (ctypes.c_void_p * 4)(base + 512, base + 640, base + 768, base + 896)
    call = lib.lfa_reduce_treev_async
    assert call(L.SUM, L.FLOAT, dst, srcs, 0, 2, None) == EINVAL
    assert call(L.SUM, L.FLOAT, dst, srcs, 33, 2, None) == EINVAL
    assert call(L.SUM, L.FLOAT, dst, None, 2, 2, None) == EINVAL
    assert call(L.SUM, L.FLOAT, None, srcs, 2, 2, None) == EINVAL
    holed = (ctypes.c_void_p * 4)(base + 512, None, base + 768, base + 896)
    assert call(L.SUM, L.FLOAT, dst, holed, 2, 2, None) == EINVAL
    over = arr([(base + 64, 8), (base + 80, 8)])
    assert call(L.SUM, L.FLOAT, over, srcs, 2, 2, None) == EINVAL
    assert call(L.BXOR, L.FLOAT, dst, srcs, 2, 2, None) == EOPNOTSUPP
    assert call(11, L.FLOAT, dst, srcs, 2, 2, None) == EOPNOTSUPP     # ATOMIC_WRITE: no tree
    assert call(L.SUM, L.FLOAT, dst, srcs, 2, 0, None) == 0
    assert np.array_equal(arena, d0)
