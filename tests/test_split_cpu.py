"""lfa_split.h without a GPU: tools/split_host_check.cpp, compiled by g++
against the header, prints the path and the head / nvec / body / tail split of
a grid of buffers and the taper split around its tile boundaries; the same
quantities are computed here from tests/_iov_layout.py's classification.  The
program is built once more with ASan + UBSan and run stand-alone."""
import os
import subprocess

import pytest

from tests import _iov_layout as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "split_host_check.cpp")
PATHS = {0: "bytes", 1: "element", 2: "vector"}
HEAD_TILE = 4096


def _build_and_run(tmp_path, name, *flags):
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                        SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    out = _build_and_run(tmp_path_factory.mktemp("split"), "split_host_check")
    return [ln.split() for ln in out.splitlines()]


def test_split_matches_model(lines):
    rows = [[int(x) for x in ln[1:]] for ln in lines if ln[0] == "split"]
    seen = set()
    for esz, doff, soff, count, path, head, nvec, body, tail in rows:
        case = (esz, doff, soff, count)
        seen.add((esz, doff, soff - doff))
        assert head + body + tail == count, case
        want = L.path(esz, count, doff, [soff])
        if want is None:        # an empty buffer: nothing anywhere, whatever the path
            assert (head, nvec, body, tail) == (0, 0, 0, 0), case
            continue
        kind, whead, wtail, _ = want
        assert PATHS[path] == kind, case
        if kind == "vector":
            assert (head, tail) == (whead, wtail), case
            assert nvec == (count - whead) * esz // 16 and body == nvec * 16 // esz, case
            if nvec:
                assert (0x10000 + doff + head * esz) % 16 == 0, case
        else:                   # no vectors: every element is element work
            assert (head, nvec, body, tail) == (count, 0, 0, 0), case
    # the grid the program walks: every element size and dst offset, src at the
    # same offset, an odd number of bytes off, and esz bytes off (esz < 16)
    for esz in (1, 2, 4, 8, 16):
        for doff in range(32):
            for delta in (0, 3) + ((esz,) if esz < 16 else ()):
                assert (esz, doff, delta) in seen
    counts = {(esz, doff): {r[3] for r in rows if r[0] == esz and r[1] == doff}
              for esz in (1, 2, 4, 8, 16) for doff in range(32)}
    for (esz, doff), got in counts.items():
        head = (16 - doff % 16) % 16 // esz
        assert {0, 1, *range(max(head - 1, 0), head + 16 // esz + 2)} <= got, (esz, doff)
    kinds = {PATHS[r[4]] for r in rows}
    assert kinds == {"bytes", "element", "vector"}


def test_taper_matches_model(lines):
    rows = [[int(x) for x in ln[1:]] for ln in lines if ln[0] == "taper"]
    want_nvec = {k * HEAD_TILE + d for k in (0, 1, 7, 8, 9) for d in (-1, 0, 1)} - {-1}
    assert {r[0] for r in rows} == want_nvec
    assert {(r[1], r[2]) for r in rows} == {(4, 256), (4, 512), (8, 256), (8, 512)}
    for nvec, div, tv, split, nhead, ntail in rows:
        case = (nvec, div, tv)
        assert split == (nvec - nvec // div) // HEAD_TILE * HEAD_TILE, case
        assert split % HEAD_TILE == 0 and nhead * HEAD_TILE == split, case
        rest = nvec - split
        assert 0 <= ntail * tv - rest < tv, case    # the tail tiles cover [split, nvec)
        assert rest >= nvec // div, case            # at least the last 1/div is tapered


def test_split_check_under_sanitizers(tmp_path, lines):
    out = _build_and_run(tmp_path, "split_host_check_san", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all")
    assert [ln.split() for ln in out.splitlines()] == lines
