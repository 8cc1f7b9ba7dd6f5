"""lfa_split.h without a GPU: tools/split_host_check.cpp, compiled by g++
against the header, prints the path and the head / nvec / body / tail split of
a grid of buffers and the taper split around its tile boundaries; the same
quantities are computed here from tests/_iov_layout.py's classification.  It
also prints the form launch_write, launch_tree_body and launch_fetch pick by size (lfa_form_*), with and without
an as_bytes override, which is held to tests/_sweep.py's model of the
launchers' table.  The program is built once more with ASan + UBSan and run
stand-alone."""
import os
import subprocess

import pytest

from tests import _iov_layout as L
from tests import _sweep as S

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


SMALL = 2597 * 16           # the sweep's body (tests/_sweep.py: lanes)
FORM_SIZES = [SMALL] + [t * S.MIB + d for t in (32, 64, 192) for d in (-16, 0, 16)] + [5 << 30]
TREE_VARIANT = {"chunk1 nt": (1, 0), "chunk2 nt": (2, 0), "lds": (3, 0), "chunk2 sc1": (11, 0),
                "chunk2 sc1 +cap": (11, 1), "put body": (25, 0)}


def test_forms_match_model(lines):
    """lfa_form_write / lfa_form_tree against the model in
    tests/_sweep.py, which is written from the table of forms and calls no C:
    at 16 bytes either side of 32, 64 and 192 MiB, at the sweep's 40 KiB and
    at 5 GiB, as the real body and as as_bytes over the 40 KiB body; write
    mapped and not, the tree at every fan-in 2..32
    and element size.  Every form appears, and without as_bytes nothing but
    the small forms below 32 MiB."""
    # the `form fetch` rows are test_fetch_forms_match_model's
    rows = [ln[1:] for ln in lines if ln[0] == "form" and ln[1] != "fetch"]
    assert {ln[1] for ln in lines if ln[0] == "form"} == {"write", "tree", "fetch"}
    seen, keys = set(), set()
    for kind, *rest in rows:
        as_bytes, real, *args = (int(x) for x in rest)
        assert real == SMALL if as_bytes else real in FORM_SIZES, rest
        nbytes = as_bytes or real
        if kind == "write":
            mapped, got = args
            form = S.model_write_form(nbytes, bool(mapped))
            assert S.WRITE_FORMS[got] == form, rest
        else:
            nsrc, nleaf, esz, variant, cap = args
            assert kind == "tree" and nleaf == S.leaves_of(nsrc) and nleaf <= nsrc < 2 * nleaf
            form = S.model_tree_form(nbytes, nsrc, esz)
            assert (variant, cap) == TREE_VARIANT[form], rest
            assert S.TREE_FORMS[variant] == form.replace(" +cap", ""), rest
        if not as_bytes and real < 32 * S.MIB:
            assert form in S.SMALL_FORMS, rest
        seen.add(form)
        keys.add((kind, bool(as_bytes), nbytes, *args[:-1 if kind != "tree" else -2]))
    assert seen == set(S.WRITE_FORMS) | set(TREE_VARIANT)
    # the grid the program walks
    for forced in (False, True):
        for nbytes in FORM_SIZES:
            assert {("write", forced, nbytes, m) for m in (0, 1)} <= keys
            assert {("tree", forced, nbytes, nsrc, S.leaves_of(nsrc), esz)
                    for nsrc in range(2, 33) for esz in (1, 2, 4, 8, 16)} <= keys
    assert len(rows) == 2 * len(FORM_SIZES) * (2 + 31 * 5)


def test_fetch_forms_match_model(lines):
    """lfa_form_fetch against tests/_sweep.py's model_fetch_form, which is
    written from launch_fetch's table of forms and calls no C: over the same
    sizes, real and forced, for 1 (ATOMIC_READ), 2 (the other readwrite ops)
    and 3 (the compare table) inputs.  Every form appears; without as_bytes
    nothing but fetch_lds below 64 MiB; at 64 MiB itself only two-input
    functors leave it."""
    rows = [[int(x) for x in ln[2:]] for ln in lines if ln[:2] == ["form", "fetch"]]
    seen, keys = set(), set()
    for as_bytes, real, nin, got in rows:
        case = (as_bytes, real, nin, got)
        assert real == SMALL if as_bytes else real in FORM_SIZES, case
        nbytes = as_bytes or real
        form = S.model_fetch_form(nbytes, nin)
        assert S.FETCH_FORMS[got] == form, case
        if not as_bytes and real < 64 * S.MIB:
            assert form == "fetch_lds sc1", case
        if nbytes == 64 * S.MIB:
            assert (form == "fetch_lds sc1") == (nin != 2), case
        seen.add(form)
        keys.add((bool(as_bytes), nbytes, nin))
    assert seen == set(S.FETCH_FORMS) and len(S.FETCH_FORMS) == 3
    assert keys == {(forced, nbytes, nin) for forced in (False, True) for nbytes in FORM_SIZES
                    for nin in (1, 2, 3)}
    assert len(FORM_SIZES) == 11 and len(rows) == 66      # 2 x 11 sizes x 3 functor shapes
    # the forced sizes of the form sweep are the thresholds themselves
    for form, as_bytes in S.FETCH_AS:
        assert S.model_fetch_form(as_bytes, 2) == form != S.model_fetch_form(as_bytes - 16, 2)


def test_split_check_under_sanitizers(tmp_path, lines):
    out = _build_and_run(tmp_path, "split_host_check_san", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all")
    assert [ln.split() for ln in out.splitlines()] == lines
