"""The fetch and compare list (fi_ioc) forms without a GPU: the exported
symbols, lfa_host_readwritev / lfa_host_swapv against the loops of
lfa_host_readwrite / lfa_host_swap for every pair of both tables, every
argument error of the four entry points (all reported before anything is
touched or enqueued, so the device forms' errors need no GPU either), the
tables built for the 3- and 4-operand records, and the stand-alone
tools/iov_host_check under ASan + UBSan."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from libfabric_amd import _native, atomic
from tests import _iov_fetch_layout as F
from tests import _iov_layout as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libfabric_amd", "csrc")
EINVAL, EOPNOTSUPP = -22, -95
INLINE = 64             # LFA_IOV_INLINE
ioc = _native.lfa_ioc
SAN = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")

# sha256 of the table lines tools/capi_host_check prints (call, seg, table,
# first, words, bound, grow: every table IovTable builds there, records of one
# and of three further pointers), taken from the build of the commit before
# the fetch and compare list forms
PARENT_TABLES = "fb0e25ace5c2529159f993a5ced6bc059393b8b88ea5544d2abf02a84a1ef140"


def _aligned(a: np.ndarray) -> np.ndarray:
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


def _build_and_run(tmp, name, srcs, *flags):
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *flags,
                        "-I" + os.path.join(ROOT, "include"), *srcs, "-lpthread", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """tools/iov_host_check's output, built with ASan + UBSan and run once."""
    srcs = [os.path.join(ROOT, "tools", "iov_host_check.cpp"), os.path.join(CSRC, "lfa_host.cpp"),
            os.path.join(CSRC, "lfa_valid.cpp")]
    return _build_and_run(tmp_path_factory.mktemp("iovf"), "iov_host_check", srcs, *SAN)


@pytest.fixture(scope="module", autouse=True)
def _forms_present():
    assert hasattr(_native.lib(), "lfa_host_swapv"), "the fetch and compare list forms are missing"


def test_symbols_exported():
    lib = _native.lib()
    for name in ("lfa_atomic_readwritev_async", "lfa_atomic_swapv_async",
                 "lfa_host_readwritev", "lfa_host_swapv"):
        assert hasattr(lib, name), name
    for name in ("readwritev", "swapv", "host_readwritev", "host_swapv"):
        assert callable(getattr(atomic, name)), name


def test_host_check_clean_under_sanitizers(host_check):
    assert "145 fetch and 84 compare parity cases and their errors pass" in host_check
    assert "25 parity cases and the overlap rule pass" in host_check


def _pairs(compare):
    ops = F.COMPARE_OPS if compare else F.FETCH_OPS
    flag = F.COMPARE_ATOMIC if compare else F.FETCH_ATOMIC
    return [(op, dt) for dt in range(16) for op in ops if atomic.atomic_valid(dt, op, flag) == 0]


def test_pair_counts():
    assert len(_pairs(False)) == 145 and len(_pairs(True)) == 84


@pytest.mark.parametrize("compare", [False, True], ids=["fetch", "compare"])
def test_host_list_form_equals_loop(compare):
    """Every valid (op, datatype): 37 segments with _iov_layout's standard counts
    and byte offsets, res a further offset on; the gaps keep their sentinel."""
    lib = _native.lib()
    names = ("dst", "src", "cmp", "res") if compare else ("dst", "src", "res")
    for op, dt in _pairs(compare):
        esz = atomic.datatype_size(dt)
        counts, offsets, _ = L.standard(37, esz, shift=op)
        assert set(counts) == set(L.COUNTS) and set(offsets) == set(L.OFFSETS)
        offs = {n: [L.OFFSETS[(L.OFFSETS.index(o) + k) % 5] for o in offsets]
                for k, n in enumerate(names)}
        ar = F.arenas(counts, offs, esz, names, 1000 + 31 * op + dt, dt)
        init = {n: a.copy() for n, (_, a) in ar.items()}
        got = {n: _aligned(a) for n, a in init.items()}
        want = {n: _aligned(a) for n, a in init.items()}
        segs = {n: s for n, (s, _) in ar.items()}
        for i in range(37):
            p = {n: want[n].ctypes.data + segs[n][i][0] for n in names}
            if compare:
                rc = lib.lfa_host_swap(op, dt, p["dst"], p["src"], p["cmp"], p["res"], counts[i])
            else:
                rc = lib.lfa_host_readwrite(op, dt, p["dst"], p["src"], p["res"], counts[i])
            assert rc == 0
        lists = [_iocs(got[n], segs[n], esz) for n in names]
        fn = lib.lfa_host_swapv if compare else lib.lfa_host_readwritev
        assert fn(op, dt, *lists, 37) == 0, (op, dt)
        for n in names:
            assert np.array_equal(got[n], want[n]), (op, dt, n)
            assert L.gaps_intact(got[n], segs[n]), (op, dt, n)
        for n in names[1:-1]:
            assert np.array_equal(got[n], init[n]), (op, dt, n)
        # res holds the old dst, segment by segment
        for (dlo, nb), (rlo, _) in zip(segs["dst"], segs["res"]):
            assert np.array_equal(got["res"][rlo:rlo + nb], init["dst"][dlo:dlo + nb]), (op, dt)
        if op != F.ATOMIC_READ:
            assert not np.array_equal(got["dst"], init["dst"]), (op, dt)


def test_host_python_forms():
    n = (5, 0, 17)
    d = [np.arange(k, dtype=np.float32) for k in n]
    s = [np.full(k, 2, np.float32) for k in n]
    r = [np.zeros(k, np.float32) for k in n]
    atomic.host_readwritev(L.SUM, L.FLOAT, d, s, r)
    for k, x, y in zip(n, d, r):
        assert np.array_equal(y, np.arange(k, dtype=np.float32))
        assert np.array_equal(x, np.arange(k, dtype=np.float32) + 2)
    r2 = [np.zeros(k, np.float32) for k in n]
    atomic.host_readwritev(F.ATOMIC_READ, L.FLOAT, d, None, r2)     # no src list
    for x, y in zip(d, r2):
        assert np.array_equal(x, y)
    c = [x.copy() for x in d]
    for x in c:
        x[1::2] = -1                    # the compare fails on the odd lanes
    atomic.host_swapv(F.CSWAP, L.FLOAT, d, s, c, r)
    for k, x, y in zip(n, d, r):
        old = np.arange(k, dtype=np.float32) + 2
        assert np.array_equal(y, old)
        old[0::2] = 2
        assert np.array_equal(x, old)
    with pytest.raises(atomic.LfaError) as e:
        atomic.host_swapv(F.MSWAP, L.FLOAT, d, s, c, r)
    assert e.value.rc == EOPNOTSUPP
    with pytest.raises(ValueError):
        atomic.host_readwritev(L.SUM, L.FLOAT, d, s[:2], r)


def _arr(items):
    a = (ioc * max(len(items), 1))()
    for i, (p, n) in enumerate(items):
        a[i].addr, a[i].count = p, n
    return a


def _error_cases(base):
    """(name, dst, src, cmp, res, nseg) — bad calls on float32 segments of one
    arena: dst from byte 0, src from 8192, cmp from 16384, res from 24576."""
    S, C, R = 8192, 16384, 24576

    def two(off, n0=8, n1=8, gap=256):
        return _arr([(base + off, n0), (base + off + gap, n1)])
    dst, src, cmp_, res = two(64), two(S), two(C), two(R)
    many = atomic.LFA_IOV_MAX + 1
    lists = [_arr([(base + o + 4 * i, 1) for i in range(many)]) for o in (64, S, C, R)]
    return [
        ("null dst array", None, src, cmp_, res, 2),
        ("null src array", dst, None, cmp_, res, 2),
        ("null res array", dst, src, cmp_, None, 2),
        ("null dst addr", _arr([(None, 8), (base + 320, 8)]), src, cmp_, res, 2),
        ("null src addr", dst, _arr([(base + S, 8), (None, 8)]), cmp_, res, 2),
        ("null res addr", dst, src, cmp_, _arr([(None, 8), (base + R + 256, 8)]), 2),
        ("src count", dst, two(S, 8, 7), cmp_, res, 2),
        ("res count", dst, src, cmp_, two(R, 9, 8), 2),
        ("too many segments", *lists, many),
        ("dst[1] overlaps dst[0]", two(64, gap=28), src, cmp_, res, 2),
        ("res[0] overlaps dst[0]", dst, src, cmp_, _arr([(base + 92, 8), (base + R, 8)]), 2),
        ("res[1] overlaps dst[0]", dst, src, cmp_, _arr([(base + R, 8), (base + 60, 8)]), 2),
        ("res[1] overlaps res[0]", dst, src, cmp_, two(R, gap=28), 2),
        ("res[1] inside res[0]", two(64, 64, 1, 1024), two(S, 64, 1, 1024), two(C, 64, 1, 1024),
         two(R, 64, 1, 128), 2),
    ]


@pytest.mark.parametrize("entry", ["lfa_host_readwritev", "lfa_atomic_readwritev_async",
                                   "lfa_host_swapv", "lfa_atomic_swapv_async"])
def test_errors_leave_buffers_untouched(entry):
    lib = _native.lib()
    compare = "swap" in entry
    a0 = np.random.default_rng(7).integers(0, 256, 24576 + 4 * atomic.LFA_IOV_MAX + 4096,
                                           dtype=np.uint8)
    arena = _aligned(a0)
    base = arena.ctypes.data
    fn = getattr(lib, entry)
    tail = (None,) if entry.endswith("async") else ()
    op = F.CSWAP if compare else L.SUM

    def call(op, dt, d, s, c, r, nseg):
        return fn(op, dt, d, s, c, r, nseg, *tail) if compare else fn(op, dt, d, s, r, nseg, *tail)
    cases = _error_cases(base)
    for name, d, s, c, r, nseg in cases:
        assert call(op, L.FLOAT, d, s, c, r, nseg) == EINVAL, name
        assert np.array_equal(arena, a0), name
    _, _, s, c, r, _ = cases[0]
    d = cases[1][1]
    if compare:
        assert call(op, L.FLOAT, d, s, None, r, 2) == EINVAL
        assert call(op, L.FLOAT, d, s, _arr([(base + 16384, 8), (None, 8)]), r, 2) == EINVAL
        assert call(op, L.FLOAT, d, s, _arr([(base + 16384, 8), (base + 16640, 9)]), r, 2) == EINVAL
    # unsupported pairs: a bitwise op on a float, the other table's ops, a
    # 16-bit float, a datatype and an op outside the tables
    bad = [(L.BXOR, L.FLOAT), (F.MSWAP if not compare else L.SUM, L.INT32), (op, 16), (op, 17),
           (op, 12), (19, L.FLOAT)]
    bad += [(F.MSWAP, L.FLOAT), (14, L.FLOAT_COMPLEX)] if compare else [(L.MIN, L.FLOAT_COMPLEX)]
    for o, dt in bad:
        assert call(o, dt, d, s, c, r, 2) == EOPNOTSUPP, (o, dt)
        assert call(o, dt, None, None, None, None, 2) == EOPNOTSUPP, (o, dt)
    assert np.array_equal(arena, a0)
    # nothing to do is not an error: no segments, or only empty ones
    assert call(op, L.FLOAT, None, None, None, None, 0) == 0
    empty = (ioc * 2)()
    assert call(op, L.FLOAT, empty, empty, empty, empty, 2) == 0
    assert np.array_equal(arena, a0)
    if tail:
        return
    # ranges that only touch are accepted (host form: it runs): dst[0] | dst[1]
    # | res[0] | res[1] back to back
    d = _arr([(base + 64, 8), (base + 96, 8)])
    r = _arr([(base + 128, 8), (base + 160, 8)])
    assert call(op, L.FLOAT, d, s, c, r, 2) == 0
    assert np.array_equal(arena[128:192], a0[64:128])
    assert np.array_equal(arena[:64], a0[:64]) and np.array_equal(arena[192:], a0[192:])
    if not compare:
        assert not np.array_equal(arena[64:128], a0[64:128])
        # ATOMIC_READ: no src list, or one of NULL addresses
        arena[:] = a0
        none = _arr([(None, 0), (None, 0)])
        for src in (None, none):
            arena[128:192] = 0
            assert call(F.ATOMIC_READ, L.FLOAT, d, src, None, r, 2) == 0
            assert np.array_equal(arena[128:192], a0[64:128])
            assert np.array_equal(arena[:128], a0[:128])


def _tabs(out):
    rows = []
    for ln in out.splitlines():
        if not ln.startswith("tab "):
            continue
        head, first, words = ln[4:].split("|")
        nin, nseg, direct, nwords = (int(x) for x in head.split())
        rows.append((nin, nseg, direct, nwords, [int(x) for x in first.split()],
                     [int(x, 16) for x in words.split()]))
    return rows


def test_fetch_and_compare_tables(host_check):
    """Word count, prefix and records of the tables with 2 (src, res) and 3
    (src, cmp, res) further pointers, and where they stop fitting the kernel
    arguments: 14 and 11 segments, as include/lfa_atomic.h says."""
    counts = (1, 4097, 3, 8192, 4096 + 5, 17)
    rows = _tabs(host_check)
    assert {(nin, nseg) for nin, nseg, *_ in rows} == {(a, b) for a in (1, 2, 3)
                                                      for b in (1, 6, 11, 14, 15)}
    fits = {}
    for nin, nseg, direct, nwords, first, words in rows:
        tiles = [L.path(4, counts[s % 6], 4, [4] * nin)[3] for s in range(nseg)]
        assert first == [sum(tiles[:s]) for s in range(nseg + 1)]
        assert direct == int(all(t == 1 for t in tiles))
        P, R = (nseg + 2) // 2, 2 + nin
        assert nwords == len(words) == P + nseg * R
        halves = [h for w in words[:P] for h in (w & 0xffffffff, w >> 32)]
        assert halves[:nseg + 1] == first and not any(halves[nseg + 1:])
        for s in range(nseg):
            rec = words[P + s * R:P + (s + 1) * R]
            assert rec == [0x10000000 + 0x100000 * s + 4, counts[s % 6],
                           *(0x100000000 * (k + 1) + 0x100000 * s + 4 for k in range(nin))]
        fits[nin, nseg] = nwords <= INLINE
    assert fits[2, 14] and not fits[2, 15] and fits[3, 11] and not fits[3, 14]
    assert max(n for n in range(1, 64) if (n + 2) // 2 + 4 * n <= INLINE) == 14
    assert max(n for n in range(1, 64) if (n + 2) // 2 + 5 * n <= INLINE) == 11


def test_writev_tables_unchanged(tmp_path):
    """The generalised record builds, for writev and treev, the bytes the
    commit before it built."""
    out = _build_and_run(tmp_path, "capi_host_check",
                         [os.path.join(ROOT, "tools", "capi_host_check.cpp"),
                          os.path.join(CSRC, "lfa_param.cpp")])
    keep = ("call", "seg", "table", "first", "words", "bound", "grow")
    lines = [ln for ln in out.splitlines() if ln.split(" ")[0] in keep]
    assert len(lines) == 283
    text = "".join(ln + "\n" for ln in lines)
    assert hashlib.sha256(text.encode()).hexdigest() == PARENT_TABLES
