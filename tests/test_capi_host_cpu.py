"""The HIP-free pieces of liblfa.so's host side without a GPU, as stand-alone
programs built by g++, plain and under ASan + UBSan:

tools/capi_host_check.cpp checks the parameter registry (lfa_param.cpp) itself
and prints the tables IovTable (lfa_iov_table.h) builds for a fixed list of
calls; they are compared here with the layout lfa_iov.h documents, tile counts
from tests/_iov_layout.py's path().  tools/iov_host_check.cpp runs the list
forms' host side against lfa_host.cpp and lfa_valid.cpp."""
import errno
import os
import subprocess

import pytest

from tests import _iov_layout as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libfabric_amd", "csrc")
CAPI = [os.path.join(ROOT, "tools", "capi_host_check.cpp"), os.path.join(CSRC, "lfa_param.cpp")]
IOV = [os.path.join(ROOT, "tools", "iov_host_check.cpp"), os.path.join(CSRC, "lfa_host.cpp"),
       os.path.join(CSRC, "lfa_valid.cpp")]
SAN = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")
INLINE = 64             # LFA_IOV_INLINE: words of a table in the kernel arguments


def _build_and_run(tmp_path, name, srcs, *flags):
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", *flags,
                        "-I" + os.path.join(ROOT, "include"), *srcs, "-lpthread", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    out = _build_and_run(tmp_path_factory.mktemp("capi"), "capi_host_check", CAPI)
    return [ln.split() for ln in out.splitlines()]


def test_registry(lines):
    # the program exits non-zero at the first registry check that fails
    assert ["registry", "ok", "64", "names"] in lines


def _calls(lines):
    """[(nin, esz, off, [(dst, count, [in])], nseg, direct, words, first, table)]"""
    out, i = [], 0
    while i < len(lines):
        if lines[i][0] != "call":
            i += 1
            continue
        nin, esz, off, n = (int(x) for x in lines[i][1:])
        segs = [(int(ln[1], 16), int(ln[2]), [int(x, 16) for x in ln[3:]])
                for ln in lines[i + 1:i + 1 + n]]
        assert all(ln[0] == "seg" for ln in lines[i + 1:i + 1 + n])
        tab, first, words = lines[i + 1 + n:i + 4 + n]
        assert (tab[0], first[0], words[0]) == ("table", "first", "words")
        out.append((nin, esz, off, segs, int(tab[1]), int(tab[2]), int(tab[3]),
                    [int(x) for x in first[1:]], [int(x, 16) for x in words[1:]]))
        i += 4 + n
    return out


def test_iov_table_layout(lines):
    calls = _calls(lines)
    seen, shapes = set(), set()
    for nin, esz, off, segs, nseg, direct, nwords, first, table in calls:
        case = (nin, esz, off, [c for _, c, _ in segs])
        seen.add((nin, esz, off))
        tiles = []
        for dst, count, ins in segs:
            assert dst % 16 == off and len(ins) == nin, case
            kind, _, _, n = L.path(esz, count, dst % 16, [a % 16 for a in ins])
            tiles.append(n)
            # (tiles, bytes in the last one): the head is ahead of tile 0's bytes
            head = 0 if kind == "bytes" else min((16 - off % 16) % 16 // esz, count)
            shapes.add((n, (count - head) * esz - (n - 1) * L.TILE))
        # first_tile[]: the prefix sum of the tile counts; direct: all are 1
        assert nseg == len(segs) and first == [sum(tiles[:s]) for s in range(nseg + 1)], case
        assert direct == int(all(n == 1 for n in tiles)), case
        # words [0, P): first_tile[] as uint32 pairs, zero padded; P = (nseg + 2) / 2
        P, R = (nseg + 2) // 2, 2 + nin
        assert nwords == len(table) == P + nseg * R, case
        halves = [h for w in table[:P] for h in (w & 0xffffffff, w >> 32)]
        assert halves[:nseg + 1] == first and not any(halves[nseg + 1:]), case
        # words [P + s·R, …): dst, count, in[0 .. nin)
        for s, (dst, count, ins) in enumerate(segs):
            assert table[P + s * R:P + (s + 1) * R] == [dst, count, *ins], case
    assert seen == {(nin, esz, off) for nin in (1, 3) for esz in (1, 4, 16) for off in (0, 4, 1)}
    assert {d for *_, d, _, _, _ in calls} == {0, 1}
    # a short tile, a tile filled to its last byte, and one element past it
    assert {(1, L.TILE), (2, 1), (2, 4), (2, 16)} <= shapes and any(
        n == 1 and last < L.TILE for n, last in shapes)


def test_iov_table_grid_bound(lines):
    (ok, rc, nseg, last), = [[int(x) for x in ln[1:]] for ln in lines if ln[0] == "bound"]
    # segments of 2^30 tiles: the sum stays at or below 2^31 - 1, so one fits
    assert ok == (2**31 - 1) // 2**30 == 1 and rc == -errno.EINVAL
    assert (nseg, last) == (ok, ok * 2**30)     # the refused segment left no trace


def test_iov_table_words_cross_inline(lines):
    rows = [[int(x) for x in ln[1:]] for ln in lines if ln[0] == "grow"]
    for nin in (1, 3):
        got = [(nseg, words, fits) for n, nseg, words, fits in rows if n == nin]
        assert [nseg for nseg, _, _ in got] == list(range(1, len(got) + 1))
        for nseg, words, fits in got:
            assert words == (nseg + 2) // 2 + nseg * (2 + nin) and fits == int(words <= INLINE)
        assert {fits for *_, fits in got} == {0, 1}     # the crossing is inside the range
    # two-word-plus-one-input records fill the inline table exactly at 18 segments
    assert (1, 18, INLINE, 1) in [tuple(r) for r in rows]


def test_capi_check_under_sanitizers(tmp_path, lines):
    out = _build_and_run(tmp_path, "capi_host_check_san", CAPI, *SAN)
    assert [ln.split() for ln in out.splitlines()] == lines


@pytest.mark.parametrize("flags", [(), SAN], ids=["plain", "asan-ubsan"])
def test_iov_host_check(tmp_path, flags):
    out = _build_and_run(tmp_path, "iov_host_check", IOV, *flags)
    assert "25 parity cases and the overlap rule pass" in out
