"""Segment layouts for the fetch and compare list-form tests, on top of
tests/_iov_layout.py: every operand of a call (dst, src, cmp, res) has an
arena of its own, carved like _iov_layout's, and its own start offsets, so a
segment's path is decided by all of its operands."""
import numpy as np

from tests import _iov_layout as L

# (enum fi_datatype, element bytes): 1-, 2-, 4-, 8- and 16-byte integers, float
INT8, INT16, INT32, INT64, INT128, FLOAT = 0, 2, 4, 6, 14, 8
DTS = (INT8, INT16, INT32, INT64, INT128, FLOAT)
ESZ = {INT8: 1, INT16: 2, INT32: 4, INT64: 8, INT128: 16, FLOAT: 4}
ATOMIC_READ, ATOMIC_WRITE, CSWAP, MSWAP = 10, 11, 12, 18
FETCH_OPS = tuple(range(12))
COMPARE_OPS = tuple(range(12, 19))
FETCH_ATOMIC, COMPARE_ATOMIC = 1 << 58, 1 << 59     # FI_FETCH_ATOMIC, FI_COMPARE_ATOMIC

NAMES = ("dst", "src", "cmp", "res")


def big(esz):
    """Three whole tiles and five elements: four tiles of dst, the last short."""
    return 3 * L.TILE // esz + 5


def layout(nseg, esz, shift=0):
    """counts and, per operand name, start offsets past a 16-byte boundary.
    Segment 0 is the multi-tile one, every operand 8 bytes past a boundary
    (the vector path with a head; 16-byte elements: offset 0).  From there on
    counts and dst offsets follow _iov_layout.standard(); res alone leaves
    dst's offset where i % 4 == 1, cmp alone (the fetch form has none: src)
    where i % 4 == 3, and segment 5 is multi-tile again on whatever path its
    offsets give."""
    counts, dst, _ = L.standard(nseg, esz, shift)
    counts, dst = list(counts), list(dst)
    counts[0], dst[0] = big(esz), 8 if esz <= 8 else 0
    if nseg > 5:
        counts[5] = big(esz)
    offs = {name: list(dst) for name in NAMES}
    for i in range(1, nseg):
        other = L.OFFSETS[(L.OFFSETS.index(dst[i]) + 1) % len(L.OFFSETS)]
        if i % 4 == 1:
            offs["res"][i] = other
        if i % 4 == 3:
            offs["cmp"][i] = offs["src"][i] = other
    return counts, offs


def paths(counts, offs, esz, names):
    """_iov_layout.path() of every segment over the operands `names` (dst first)."""
    return [L.path(esz, c, offs["dst"][i], [offs[n][i] for n in names[1:]])
            for i, c in enumerate(counts)]


def assert_paths(seen):
    """`seen`: {esz: [path() of every non-empty segment]} over all six
    datatypes.  Each path occurs wherever the element size allows it (a 1-byte
    element is never misaligned; 16-byte elements that are aligned are
    co-aligned and have neither head nor tail), and the vector path carries a
    head, a tail and a segment of at least three tiles."""
    for esz, ps in seen.items():
        kinds = {p[0] for p in ps}
        want = {"vector", "element", "bytes"} - {"bytes" if esz == 1 else "",
                                                 "element" if esz == 16 else ""}
        assert kinds == want, (esz, kinds)
        vec = [p for p in ps if p[0] == "vector"]
        assert any(tiles >= 3 for *_, tiles in vec), esz
        if esz < 16:
            assert any(head for _, head, _, _ in vec) and any(tail for _, _, tail, _ in vec), esz
            assert any(head and tiles >= 3 for _, head, _, tiles in vec), esz


def arenas(counts, offs, esz, names, seed, dt):
    """{name: (segs, bytes)}: a filled arena per operand.  Every other element
    of cmp is dst's, so each compare holds on some lanes and fails on others."""
    out = {}
    for k, name in enumerate(names):
        segs, size = L.plan(counts, offs[name], esz)
        out[name] = (segs, L.fill(size, segs, seed + 17 * k, dt))
    if "cmp" in out:
        (dsegs, d), (csegs, c) = out["dst"], out["cmp"]
        for (dlo, nb), (clo, _) in zip(dsegs, csegs):
            dv = d[dlo:dlo + nb].reshape(-1, esz)
            c[clo:clo + nb].reshape(-1, esz)[::2] = dv[::2]
    return out


def valid_ops(atomic, dt, compare):
    ops, flag = (COMPARE_OPS, COMPARE_ATOMIC) if compare else (FETCH_OPS, FETCH_ATOMIC)
    return [op for op in ops if atomic.atomic_valid(dt, op, flag) == 0]


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)
