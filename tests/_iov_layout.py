"""Segment layouts for the list-form (fi_ioc) tests: every segment of a call
carved from one arena, 64 sentinel bytes between neighbours, each segment's
start a chosen number of bytes past a 16-byte boundary."""
import numpy as np

SENTINEL = 0xC3
GAP = 64
COUNTS = (0, 1, 3, 15, 16, 17, 255, 4097)
OFFSETS = (0, 1, 2, 4, 8)

# (enum fi_datatype, element bytes)
INT8, FLOAT, DOUBLE, FLOAT_COMPLEX, INT128, BFLOAT16 = 0, 8, 9, 10, 14, 17
INT32, INT64 = 4, 6
ESZ = {INT8: 1, INT32: 4, INT64: 8, FLOAT: 4, DOUBLE: 8, FLOAT_COMPLEX: 8, INT128: 16,
       BFLOAT16: 2}
INTEGERS = (INT8, INT32, INT64, INT128)
MIN, SUM, PROD, LXOR, BXOR = 0, 2, 3, 8, 9


def plan(counts, offsets, esz):
    """[(start byte, byte length)] for segments of counts[i] elements, segment i
    starting offsets[i] bytes past a 16-byte boundary, and the arena's size."""
    segs, pos = [], GAP
    for n, off in zip(counts, offsets):
        pos = (pos + 15) // 16 * 16 + off
        segs.append((pos, n * esz))
        pos += n * esz + GAP
    return segs, pos + 16


def standard(nseg, esz, shift=0):
    """Counts drawn from COUNTS and starts from OFFSETS: empty, sub-vector,
    one-vector, odd and multi-tile segments at every kind of misalignment."""
    counts = [COUNTS[(i * 3 + shift) % len(COUNTS)] for i in range(nseg)]
    offsets = [OFFSETS[(i + shift) % len(OFFSETS)] for i in range(nseg)]
    return counts, offsets, plan(counts, offsets, esz)


TILE = 16384            # LFA_IOV_TILE: bytes of dst per workgroup


def path(esz, count, dst_off, in_offs):
    """How the list kernels treat one segment whose dst starts dst_off bytes
    and whose inputs start in_offs bytes past a 16-byte boundary: None for an
    empty segment, else (path, head, tail, tiles) with path one of "vector",
    "element", "bytes"; head and tail are the elements before dst's first and
    after its last whole 16-byte vector (vector path only, else 0)."""
    if not count:
        return None
    offs = [dst_off, *in_offs]
    if any(o % esz for o in offs):
        return "bytes", 0, 0, -(-count * esz // TILE)
    head = min((16 - dst_off % 16) % 16 // esz, count)
    tiles = max(1, -(-(count - head) * esz // TILE))
    if any((o - dst_off) % 16 for o in in_offs):
        return "element", 0, 0, tiles
    return "vector", head, (count - head) * esz % 16 // esz, tiles


def fill(size, segs, seed, dt=None):
    """An arena of `size` bytes: sentinel everywhere, seeded data in the
    segments (small exact values for the float types with NaN and inf
    lanes among them; random bytes otherwise)."""
    rng = np.random.default_rng(seed)
    a = np.full(size, SENTINEL, np.uint8)

    def special(v):                 # some NaN and inf lanes among the values
        v[5::7] = np.nan
        v[3::11] = np.inf
        return v
    for lo, nb in segs:
        if dt in (FLOAT, FLOAT_COMPLEX):
            v = special(rng.integers(-8, 9, nb // 4).astype(np.float32) / 4)
            a[lo:lo + nb] = v.view(np.uint8)
        elif dt == DOUBLE:
            a[lo:lo + nb] = special(rng.integers(-8, 9, nb // 8).astype(np.float64) / 4).view(np.uint8)
        elif dt == BFLOAT16:
            v = special(rng.integers(-8, 9, nb // 2).astype(np.float32) / 4)
            a[lo:lo + nb] = (v.view(np.uint32) >> 16).astype(np.uint16).view(np.uint8)
        else:
            a[lo:lo + nb] = rng.integers(0, 256, nb, dtype=np.uint8)
    return a


def gaps_intact(arena, segs):
    """Every byte outside the segments still holds the sentinel."""
    mask = np.ones(arena.size, bool)
    for lo, nb in segs:
        mask[lo:lo + nb] = False
    return bool((np.asarray(arena)[mask] == SENTINEL).all())


# standard()'s shift per element size at which tree_layout() puts on the
# vector path a multi-tile segment that is its own input, segments with a
# head and with a tail, and (8-byte elements, where 4097 elements past a head
# still span two tiles) a multi-tile segment with a head
TREE_SHIFT = {2: 1, 4: 3, 8: 39,
              # tests/_sweep.py (assert_treev_paths): a 1-byte element is never
              # misaligned and one tile holds 4097 of them; a 16-byte element
              # is on the vector path only at offset 0, where shift 3 puts the
              # 4097-element segment that is its own input
              1: 1, 16: 3}


def tree_layout(esz, nsrc):
    """19 segments for the tree form; input k of segment i starts where dst[i]
    does when i % 4 < 2 or k is even, else where dst[i + 1] does, and dst[i]
    is its own input 0 for even i.  So from two inputs on every path (vector,
    element, byte-wise) carries aliased and unaliased segments.
    Returns dst's (segs, size), [(segs, size)] per input and, per segment,
    (path(), dst is its own input)."""
    counts, offsets, (segs, size) = standard(19, esz, shift=TREE_SHIFT[esz])
    n = len(counts)
    offs = [[offsets[i] if i % 4 < 2 or k % 2 == 0 else offsets[(i + 1) % n]
             for i in range(n)] for k in range(nsrc)]
    paths = []
    for i in range(n):
        ins = [offsets[i] if k == 0 and i % 2 == 0 else offs[k][i] for k in range(nsrc)]
        paths.append((path(esz, counts[i], offsets[i], ins), i % 2 == 0))
    return segs, size, [plan(counts, o, esz) for o in offs], paths


def assert_tree_paths(esz, paths):
    """tree_layout()'s segments reach each path of the tree kernel, and on the
    vector path every shape that has code of its own."""
    paths = [(p, own) for p, own in paths if p]
    for kind in ("vector", "element", "bytes"):
        assert {own for p, own in paths if p[0] == kind} == {True, False}, kind
    vec = [(head, tail, tiles, own) for (kind, head, tail, tiles), own in paths
           if kind == "vector"]
    assert any(head for head, *_ in vec) and any(tail for _, tail, *_ in vec)
    if esz >= 4:            # 4097 two-byte elements are one tile
        assert any(tiles > 1 and own for *_, tiles, own in vec)
        assert any(tiles > 1 and tail for _, tail, tiles, _ in vec)
    if esz == 8:
        assert any(tiles > 1 and head for head, _, tiles, _ in vec)
