"""The oracle sweep's cases and inputs: no GPU, no product code.

tests/test_sweep_gpu.py runs every (op, datatype) pair through every tree,
tree-put and list-form kernel instantiation liblfa.so holds,
tests/test_sweep_tables_gpu.py every entry of the write, fetch and compare
tables through its own kernels, tests/test_sweep_forms_gpu.py every form the
write and tree launchers only take at large sizes (the last parts of this module);
tests/test_sweep_cpu.py runs the same cases through the host forms and
checks the conditions below on the inputs themselves.  This module builds the
cases: the pair lists, operands whose result depends on EVERY input, the byte
offsets that send a launcher down each of its paths, and one arena per case
(64 sentinel bytes between operands, tests/_iov_layout.py's convention) from
which every operand is carved, so a case is one upload and one download and a
write outside any operand shows.

Why not the random operands of the other tree tests: at wide fan-in they go
blind.  BAND of 32 uniform integers is 0 on practically every lane, BOR all
ones, integer PROD 0 mod 2^k, LAND / LOR constant, so a body that dropped or
duplicated a leaf would still pass.  `inputs` below keeps every input
visible in the result at 32 inputs (tests/test_sweep_cpu.py holds it to that).
"""
import numpy as np

import oracle
from tests import _half_ref as R
from tests import _iov_layout as L
from tests._cmp import assert_parity

MIN, MAX, SUM, PROD, LOR, LAND, BOR, BAND, LXOR, BXOR, READ, WRITE = range(12)
HALF = (R.FLOAT16, R.BFLOAT16)
HALF_REDUCE_OPS = (MIN, MAX, SUM, PROD, LOR, LAND, LXOR)

# What the sweep must cover.  Literals: the tests compare them with the lists
# built below and with atomic.reduce_valid, so a pair that silently left a
# list fails instead of shrinking the sweep.
N_REDUCE_PAIRS = 133        # 119 table entries (ops 0..9) + 2 half types x 7 ops
N_WRITE_PAIRS = 148         # the 132 golden combine entries + 2 half types x 8 ops

TREE_NSRC = (2, 3, 5, 8, 9, 17, 32)
PUT_NSRC = (1, 3, 5, 9, 17, 32)
PUT_NDST = (2, 6)
# 2 and 3 inputs: reduce_iov's 2-leaf body; 5: the 4-leaf one; 8 and 15: 8 leaves
TREEV_NSRC = (2, 3, 5, 8, 15)
TREE_ALIAS = ("highest", "input0")
PATHS = ("vec", "head", "elem", "bytes")
# paths a launcher can take per element size: a 1-byte element is never
# misaligned; a 16-byte element that is aligned is co-aligned
N_PATHS = {1: 3, 2: 4, 4: 4, 8: 4, 16: 2}

OUT_FILL = 0x3C             # an output before the call (neither sentinel nor 0)


def np_dtype(dt: int) -> np.dtype:
    return np.dtype(np.uint16) if dt in HALF else oracle.DT_NP[dt]


def esz_of(dt: int) -> int:
    return np_dtype(dt).itemsize


def reduce_pairs():
    """(op, dt) of every reducing instantiation, op-major."""
    table = [(op, dt) for op in range(10) for dt in oracle.DT_NP if oracle.has_handler(op, dt)]
    half = [(op, dt) for op in HALF_REDUCE_OPS for dt in HALF]
    return sorted(table + half)


def write_pairs(manifest):
    """(op, dt) of every binary list-form instantiation: the golden manifest's
    combine entries plus the half types' write rows."""
    table = [(c["op"], c["dt"]) for c in manifest["combine"]]
    half = [(op, dt) for op in R.OPS for dt in HALF]
    return sorted(table + half)


def dts_of(op: int):
    return [dt for o, dt in reduce_pairs() if o == op]


def paths_of(esz: int):
    return [p for p in PATHS
            if not (p in ("head", "elem") and esz >= 16) and not (p == "bytes" and esz == 1)]


# ------------------------------------------------------------- reference --

def reference(op: int, dt: int, ins) -> np.ndarray:
    """prov/coll's tree over `ins` (byte arrays), as bytes."""
    if dt in HALF:
        return R.tree(dt, op, [np.ascontiguousarray(x).view(np.uint16) for x in ins]).view(np.uint8)
    nd = oracle.DT_NP[dt]
    return oracle.allreduce(op, dt, [np.ascontiguousarray(x).view(nd).copy()
                                     for x in ins])[0].view(np.uint8)


def reference_write(op: int, dt: int, dst, src) -> np.ndarray:
    """dst OP src (byte arrays), as bytes."""
    if dt in HALF:
        return R.step(dt, op, np.ascontiguousarray(dst).view(np.uint16),
                      np.ascontiguousarray(src).view(np.uint16)).view(np.uint8)
    nd = oracle.DT_NP[dt]
    d = np.ascontiguousarray(dst).view(nd).copy()
    if d.size:
        oracle.write(op, dt, d, np.ascontiguousarray(src).view(nd).copy())
    return d.view(np.uint8)


def assert_same(dt: int, got, want, what: str) -> None:
    if dt in HALF:
        R.assert_half(dt, np.ascontiguousarray(got).view(np.uint16),
                      np.ascontiguousarray(want).view(np.uint16), what)
    else:
        assert_parity(dt, got, want, what)


def nan_lanes(dt: int, b) -> np.ndarray:
    """Per element: is any component NaN (float, complex and half types)."""
    b = np.ascontiguousarray(b)
    if dt in HALF:
        return R.isnan(dt, b.view(np.uint16))
    nd = oracle.DT_NP[dt]
    if nd.kind == "c":
        v = b.view(nd)
        return np.isnan(v.real) | np.isnan(v.imag)
    return np.isnan(b.view(nd))


def is_float(dt: int) -> bool:
    return dt in HALF or oracle.DT_NP[dt].kind in "fc"


# ---------------------------------------------------------------- inputs --

EDGE_LANES = 64


def _edges(dt: int):
    """The edge values of dt, or None (int128): +-0, +-inf, NaN of either
    sign, the smallest normal, +-smallest subnormal, +-largest finite and +-1
    for the float types (every pair of them for complex, _half_ref.SPECIALS
    for the half types); min, max, 0, 1, max - 1 and -1 for the integers."""
    if dt in HALF:
        return np.array(R.SPECIALS[dt], np.uint16)
    nd = oracle.DT_NP[dt]
    if nd.kind == "V":
        return None
    if nd.kind == "c":
        f = _edges(oracle.DT_CODE["FLOAT"])
        c = np.empty(f.size * f.size, nd)
        c.real, c.imag = np.repeat(f, f.size), np.tile(f[::-1], f.size)
        return c
    if nd.kind == "f":
        fi = np.finfo(nd)
        return np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, fi.tiny,
                         fi.smallest_subnormal, -fi.smallest_subnormal, fi.max, -fi.max,
                         1.0, -1.0], dtype=nd)
    ii = np.iinfo(nd)
    return np.array([ii.min, ii.max, 0, 1, ii.max - 1] + ([-1] if ii.min < 0 else []), dtype=nd)


def _floats(dt: int, f: np.ndarray) -> np.ndarray:
    """float64 values -> (n, esz) bytes of dt (complex: pairs of values)."""
    if dt in HALF:
        x = R.from_float(dt, f)
    else:
        nd = oracle.DT_NP[dt]
        x = f.astype(np.float32).view(np.complex64) if nd.kind == "c" else f.astype(nd)
    return x.view(np.uint8).reshape(-1, esz_of(dt)).copy()


def inputs(op: int, dt: int, nsrc: int, n: int, rng) -> list:
    """nsrc operands of n elements (byte arrays) whose result under `op`
    depends on every one of them.

    SUM, float / complex PROD: magnitudes 0.5..1.5 with a random sign;
    integers uniform.  Integer PROD: odd factors, so the wrapped product
    keeps every bit.  MIN / MAX: uniform, and for the float types every input
    holds +0 or -0 on a tenth of the lanes (the result there is decided by
    the association order alone).  BAND: all ones, except that per lane one
    input holds a random mask; BOR the mirror image over zeros.  LAND: every
    input nonzero, except that on half the lanes one input is zero; LOR the
    mirror image.  LXOR: each lane zero with probability 1/2; BXOR uniform.
    ATOMIC_WRITE takes SUM's.  The last 64 lanes of every input hold edge
    values (NaN, +-inf, subnormals, type extremes), so the bulk stays finite.
    """
    esz = esz_of(dt)
    flt = is_float(dt)
    comp = 2 if (dt not in HALF and oracle.DT_NP[dt].kind == "c") else 1
    xs = []
    for _ in range(nsrc):
        if flt and op in (MIN, MAX):
            x = _floats(dt, rng.uniform(-2.0, 2.0, n * comp))
        elif flt:
            x = _floats(dt, rng.uniform(0.5, 1.5, n * comp) * rng.choice([-1.0, 1.0], n * comp))
        else:
            x = rng.integers(0, 256, (n, esz), dtype=np.uint8)      # uniform over the type
        xs.append(x)
    who = rng.integers(0, nsrc, n)          # per lane: the input that differs
    half = rng.random(n) < 0.5
    if op == PROD and not flt:
        for x in xs:
            x[:, 0] |= 1
    elif op in (MIN, MAX) and flt:
        zero = rng.random(n) < 0.1
        for x in xs:
            x[zero] = 0
            if dt in HALF:      # the sign bit of random 16-bit patterns
                sign = (R.patterns(n, int(rng.integers(0, 2**31))) >> 8).astype(np.uint8) & 0x80
            else:
                sign = rng.choice(np.array([0, 0x80], np.uint8), n)
            x[zero, esz - 1] = sign[zero]
    elif op in (BAND, BOR):
        mask = rng.integers(0, 256, (n, esz), dtype=np.uint8)
        rest = 0xFF if op == BAND else 0
        for k, x in enumerate(xs):
            x[:] = np.where((who == k)[:, None], mask, np.uint8(rest))
    elif op in (LAND, LOR):
        for k, x in enumerate(xs):
            if not flt:
                x[:, 0] |= 1                # nonzero
            odd = (who == k) & half         # the lane's one zero (LAND) / nonzero (LOR)
            x[odd if op == LAND else ~odd] = 0
    elif op == LXOR:
        for x in xs:
            if not flt:
                x[:, 0] |= 1
            x[rng.random(n) < 0.5] = 0
    ev = _edges(dt)
    ne = min(EDGE_LANES, n)
    if ev is not None and ne:
        eb = np.ascontiguousarray(ev).view(np.uint8).reshape(-1, esz)
        for x in xs:
            x[n - ne:] = eb[rng.integers(0, eb.shape[0], ne)]
    return [x.reshape(-1) for x in xs]


# ---------------------------------------------------------------- layout --

def lanes(esz: int) -> int:
    """The smallest count that gives the widest body (16 KiB of output per
    workgroup: reduce_tree_put with U = 4, combine_iov) two whole workgroup
    tiles, a partial tile, a partial wave and a ragged tail."""
    return (40 * 1024 + 16 * 37) // esz + 3


def layout(esz: int, path: str, ndst: int = 1, nsrc: int = 2):
    """(n, output offsets, input offsets): where each operand starts, in bytes
    past a 16-byte boundary, for a launcher to take `path`.

    vec    every operand 16-byte aligned: vector body, a partial wave, a tail
    head   every operand esz bytes past a boundary, co-aligned: the tree takes
           the element kernel for the whole buffer, the put form peels a head
    elem   input 1 one element further on than the rest (with one input: the
           last output): element path
    bytes  output 0 and input 0 one byte off: bytes path
    """
    assert path in paths_of(esz), (esz, path)
    outs, ins = [0] * ndst, [0] * nsrc
    if path == "head":
        outs, ins = [esz] * ndst, [esz] * nsrc
    elif path == "elem":
        if nsrc > 1:
            ins[1] = esz
        else:
            assert ndst > 1
            outs[-1] = esz
    elif path == "bytes":
        outs[0] = ins[0] = 1
    return lanes(esz), outs, ins


def expect_path(esz: int, outs, ins) -> str:
    """lfa_split.h's rule on the offsets: which path a launcher takes."""
    offs = list(outs) + list(ins)
    if any(o % esz for o in offs):
        return "bytes"
    if any((o - outs[0]) % 16 for o in offs) or esz > 16:
        return "elem"
    return "head" if outs[0] % 16 else "vec"


class Case:
    """One call's operands in one arena.  `outs` / `ins`: (start, bytes) per
    operand; an aliased output is the same range as its input.  `want`: the
    bytes every output must hold afterwards."""

    def __init__(self, arena, outs, ins, want, what, segs):
        self.arena, self.outs, self.ins = arena, outs, ins
        self.want, self.what, self.segs = want, what, segs

    def check(self, dt: int, got: np.ndarray) -> None:
        got = np.asarray(got)
        assert got.shape == self.arena.shape, self.what
        assert L.gaps_intact(got, self.segs), f"{self.what}: a gap lost its sentinel"
        for k, (lo, nb) in enumerate(self.ins):
            if (lo, nb) not in self.outs:
                assert np.array_equal(got[lo:lo + nb], self.arena[lo:lo + nb]), \
                    f"{self.what}: input {k} changed"
        for j, (lo, nb) in enumerate(self.outs):
            assert_same(dt, got[lo:lo + nb].copy(), self.want, f"{self.what} out {j}")


def carve(dt, data, want, path, ndst=1, alias=None, what=""):
    """A Case for the operands `data` on `path` with ndst outputs; alias:
    None, "highest" or "input0": the one output IS that input."""
    esz, nsrc = esz_of(dt), len(data)
    n, o_off, i_off = layout(esz, path, 0 if alias else ndst, nsrc)
    assert n * esz == data[0].size
    assert expect_path(esz, o_off or [i_off[-1 if alias == "highest" else 0]], i_off) == path
    segs, size = L.plan([n] * (len(o_off) + nsrc), o_off + i_off, esz)
    arena = np.full(size, L.SENTINEL, np.uint8)
    outs, ins = segs[:len(o_off)], segs[len(o_off):]
    for lo, nb in outs:
        arena[lo:lo + nb] = OUT_FILL
    for (lo, nb), x in zip(ins, data):
        arena[lo:lo + nb] = x
    if alias:
        outs = [ins[-1 if alias == "highest" else 0]]
    return Case(arena, outs, ins, want, what, segs)


def tree_cases(op, dt, rng, nsrcs=TREE_NSRC):
    """Every case of the single-call tree for one pair: each fan-in on each
    path, and on the vec path once more with the output aliasing the highest
    input and once with it aliasing input 0."""
    esz = esz_of(dt)
    for nsrc in nsrcs:
        data = inputs(op, dt, nsrc, lanes(esz), rng)
        want = reference(op, dt, data)
        for path in paths_of(esz):
            yield carve(dt, data, want, path, what=f"tree op={op} dt={dt} nsrc={nsrc} {path}")
        for alias in TREE_ALIAS:
            yield carve(dt, data, want, "vec", alias=alias,
                        what=f"tree op={op} dt={dt} nsrc={nsrc} out is {alias}")


def n_tree_cases(op) -> int:
    return sum(len(TREE_NSRC) * (N_PATHS[esz_of(dt)] + len(TREE_ALIAS)) for dt in dts_of(op))


def put_cases(op, dt, rng):
    """(ndst, Case) of the tree-put form for one pair."""
    esz = esz_of(dt)
    for nsrc in PUT_NSRC:
        data = inputs(op, dt, nsrc, lanes(esz), rng)
        want = reference(op, dt, data)
        for path in paths_of(esz):
            for ndst in PUT_NDST:
                yield carve(dt, data, want, path, ndst=ndst,
                            what=f"put op={op} dt={dt} nsrc={nsrc} ndst={ndst} {path}")


def n_put_cases(op) -> int:
    return sum(len(PUT_NSRC) * N_PATHS[esz_of(dt)] * len(PUT_NDST) for dt in dts_of(op))


# ------------------------------------------------------------ list forms --

class ListCase:
    """A list-form call: every arena of the call back to back in ONE buffer
    (`arena`), each from a 256-byte boundary.  dst[i] / src[k][i]: (start,
    bytes) in that buffer; want[i]: segment i's bytes afterwards."""

    def __init__(self, arena, dst, src, want, what):
        self.arena, self.dst, self.src = arena, dst, src
        self.want, self.what = want, what

    def check(self, dt: int, got: np.ndarray) -> None:
        got = np.asarray(got)
        keep = np.ones(got.size, bool)
        for lo, nb in self.dst:
            keep[lo:lo + nb] = False
        # every gap, every input and every input arena's unused bytes
        assert np.array_equal(got[keep], self.arena[keep]), \
            f"{self.what}: bytes outside the dst segments changed"
        for i, (lo, nb) in enumerate(self.dst):
            assert_same(dt, got[lo:lo + nb].copy(), self.want[i], f"{self.what} seg {i}")


def _pack(arenas):
    """Arenas back to back from 256-byte boundaries: the buffer, each base."""
    bases, pos = [], 0
    for a in arenas:
        bases.append(pos)
        pos += (a.size + 255) // 256 * 256
    big = np.full(pos, L.SENTINEL, np.uint8)
    for b, a in zip(bases, arenas):
        big[b:b + a.size] = a
    return big, bases


def _split(x, counts, esz):
    cuts = np.cumsum([0] + [c * esz for c in counts])
    return [x[cuts[i]:cuts[i + 1]] for i in range(len(counts))]


def writev_kinds(esz):
    return {"vector", "element", "bytes"} - {"bytes" if esz == 1 else "",
                                             "element" if esz == 16 else ""}


def writev_case(op, dt, rng):
    """37 segments (_iov_layout.standard): vector, element and bytes segments
    in one call; every third source starts where the next segment's dst does."""
    esz, nseg = esz_of(dt), 37
    counts, offsets, (segs, size) = L.standard(nseg, esz, shift=op)
    soffs = [offsets[(i + 1) % nseg] if i % 3 == 2 else o for i, o in enumerate(offsets)]
    ssegs, ssize = L.plan(counts, soffs, esz)
    kinds = {p[0] for p in (L.path(esz, c, o, [so])
                            for c, o, so in zip(counts, offsets, soffs)) if p}
    assert kinds == writev_kinds(esz), (esz, kinds)
    d, s = inputs(SUM if op == WRITE else op, dt, 2, sum(counts), rng)
    da, sa = np.full(size, L.SENTINEL, np.uint8), np.full(ssize, L.SENTINEL, np.uint8)
    want = []
    for (lo, nb), (slo, _), dseg, sseg in zip(segs, ssegs, _split(d, counts, esz),
                                              _split(s, counts, esz)):
        da[lo:lo + nb], sa[slo:slo + nb] = dseg, sseg
        want.append(reference_write(op, dt, dseg, sseg))
    big, (db, sb) = _pack([da, sa])
    return ListCase(big, [(db + lo, nb) for lo, nb in segs], [[(sb + lo, nb) for lo, nb in ssegs]],
                    want, f"writev op={op} dt={dt}")


def assert_treev_paths(esz, paths):
    """tree_layout()'s segments reach every path the element size has, each
    with aliased and unaliased segments (_iov_layout.assert_tree_paths is the
    full statement for the sizes that have all three)."""
    if esz in (2, 4, 8):
        L.assert_tree_paths(esz, paths)
        return
    paths = [(p, own) for p, own in paths if p]
    for kind in ("vector", "element", "bytes"):
        owns = {own for p, own in paths if p[0] == kind}
        assert owns == ({True, False} if kind in writev_kinds(esz) else set()), (esz, kind)
    vec = [(head, tail, tiles, own) for (kind, head, tail, tiles), own in paths
           if kind == "vector"]
    if esz == 1:
        assert any(head for head, *_ in vec) and any(tail for _, tail, *_ in vec)
    else:       # 4097 sixteen-byte elements: four tiles and a fifth, partial one
        assert any(tiles > 1 and own for *_, tiles, own in vec)


def treev_case(op, dt, nsrc, rng):
    """_iov_layout.tree_layout's 19 segments; dst[i] is its own input 0 for
    even i."""
    esz = esz_of(dt)
    segs, size, in_k, paths = L.tree_layout(esz, nsrc)
    assert_treev_paths(esz, paths)
    counts = [nb // esz for _, nb in segs]
    data = [_split(x, counts, esz) for x in inputs(op, dt, nsrc, sum(counts), rng)]
    nseg = len(segs)
    da = np.full(size, L.SENTINEL, np.uint8)
    for i, (lo, nb) in enumerate(segs):
        da[lo:lo + nb] = data[0][i] if i % 2 == 0 else OUT_FILL
    arenas = [da]
    for k, (sk, size_k) in enumerate(in_k):
        a = np.full(size_k, L.SENTINEL, np.uint8)
        for i, (lo, nb) in enumerate(sk):
            a[lo:lo + nb] = data[k][i]
        arenas.append(a)
    big, bases = _pack(arenas)
    dst = [(bases[0] + lo, nb) for lo, nb in segs]
    src = [[(bases[1 + k] + lo, nb) for lo, nb in in_k[k][0]] for k in range(nsrc)]
    for i in range(0, nseg, 2):
        src[0][i] = dst[i]
    want = [reference(op, dt, [data[k][i] for k in range(nsrc)]) if counts[i]
            else np.zeros(0, np.uint8) for i in range(nseg)]
    return ListCase(big, dst, src, want, f"treev op={op} dt={dt} nsrc={nsrc}")


# --------------------------------------------------------- binary tables --
# The three tables' own kernels: lfa_atomic_write_async (launch_write:
# combine_lds / combine_elem / combine_unaligned), lfa_atomic_readwrite_async
# and lfa_atomic_swap_async (launch_fetch: fetch_lds / fetch_elem with the
# ALIGNED and the byte-wise functor).  Both launchers cut 16-KiB workgroup
# tiles (4 waves x 4 KiB), so lanes() gives them two whole tiles, a partial
# tile with whole and partial waves, and a ragged tail.

CSWAP, CSWAP_NE, CSWAP_LE, CSWAP_LT, CSWAP_GE, CSWAP_GT, MSWAP = range(12, 19)
N_RW_PAIRS = 145            # 119 entries of ops 0..9 + 13 ATOMIC_READ + 13 ATOMIC_WRITE
N_SWAP_PAIRS = 84           # 2 x 13 (CSWAP, CSWAP_NE) + 4 x 12 ordered + 10 MSWAP
WRITE_OPS = tuple(op for op in range(12) if op != READ)
RW_OPS = tuple(range(12))
SWAP_OPS = tuple(range(12, 19))

# operands in the order the launcher classifies them (dst first)
TABLE_OPERANDS = {"write": ("dst", "src"), "readwrite": ("dst", "res", "src"),
                  "read": ("dst", "res"), "swap": ("dst", "src", "cmp", "res")}
# who may be the one operand off the others' alignment, rotated by case index
ODD = {"elem": ("src", "res", "cmp"), "bytes": ("src", "res", "cmp", "dst")}


def rw_pairs():
    return [(op, dt) for op in RW_OPS for dt in oracle.DT_NP if oracle.has_readwrite(op, dt)]


def swap_pairs():
    return [(op, dt) for op in SWAP_OPS for dt in oracle.DT_NP if oracle.has_swap(op, dt)]


def table_dts(pairs, op):
    return [dt for o, dt in pairs if o == op]


def n_table_cases(dts, paths=PATHS) -> int:
    return sum(len([p for p in paths_of(esz_of(dt)) if p in paths]) for dt in dts)


def table_layout(esz: int, path: str, names, k: int = 0):
    """(byte offsets past a 16-byte boundary per operand of `names`, the odd
    operand or None) for launch_write / launch_fetch to take `path`.

    vec    every operand 16-byte aligned
    head   every operand esz bytes past a boundary: element head, vector
           body, and the element tail the size then leaves (the vec path's
           tail is there at every element size below 16)
    elem   one operand (src, res or cmp: the k-th of those the call has) one
           element further on than the rest: fetch_elem / combine_elem alone
    bytes  one operand (those and dst) one byte off: the byte-wise functor
    """
    assert path in paths_of(esz), (esz, path)
    offs = dict.fromkeys(names, esz if path == "head" else 0)
    odd = None
    if path in ODD:
        cands = [o for o in ODD[path] if o in names]
        odd = cands[k % len(cands)]
        offs[odd] = esz if path == "elem" else 1
    order = [offs[o] for o in names]
    assert expect_path(esz, order[:1], order[1:]) == path, (esz, path, names, odd)
    return order, odd


def reference_readwrite(op: int, dt: int, dst, src) -> np.ndarray:
    """The new dst of oracle.readwrite (byte arrays; src None: ATOMIC_READ)."""
    nd = oracle.DT_NP[dt]
    d = np.ascontiguousarray(dst).view(nd).copy()
    s = np.ascontiguousarray(dst if src is None else src).view(nd).copy()
    r = np.zeros_like(d)
    oracle.readwrite(op, dt, d, s, r)
    assert np.array_equal(r.view(np.uint8), np.ascontiguousarray(dst)), "oracle: res != old dst"
    return d.view(np.uint8)


def reference_swap(op: int, dt: int, dst, src, cmp) -> np.ndarray:
    """The new dst of oracle.swap's shipping (CAS) variant (byte arrays)."""
    nd = oracle.DT_NP[dt]
    d = np.ascontiguousarray(dst).view(nd).copy()
    r = np.zeros_like(d)
    oracle.swap(op, dt, d, np.ascontiguousarray(src).view(nd).copy(),
                np.ascontiguousarray(cmp).view(nd).copy(), r, oracle.CAS)
    assert np.array_equal(r.view(np.uint8), np.ascontiguousarray(dst)), "oracle: res != old dst"
    return d.view(np.uint8)


# ----------------------------------------------------------- swap inputs --

def is_complex(dt: int) -> bool:
    return dt not in HALF and oracle.DT_NP[dt].kind == "c"


def _signed(dt: int) -> bool:
    return oracle.DT_NP[dt].kind == "i" or dt == oracle.DT_CODE["INT128"]


def _draw(dt: int, n: int, rng) -> np.ndarray:
    """n values of dt as (n, esz) bytes: integers uniform over the type,
    floats (each component of a complex) uniform in (-2, 2)."""
    if is_float(dt):
        return _floats(dt, rng.uniform(-2.0, 2.0, n * (2 if is_complex(dt) else 1)))
    return rng.integers(0, 256, (n, esz_of(dt)), dtype=np.uint8)


def values_equal(dt: int, a, b) -> np.ndarray:
    """Per lane: a == b as VALUES of dt (+0 == -0, NaN != NaN)."""
    nd = oracle.DT_NP[dt]
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    if nd.kind in "fc":
        return a.view(nd) == b.view(nd)
    return (a.reshape(-1, nd.itemsize) == b.reshape(-1, nd.itemsize)).all(axis=1)


def _less(dt: int, a, b) -> np.ndarray:
    """Per lane: a < b.  int128 / uint128 as (high, low) 64-bit words, the
    high word signed for INT128."""
    nd = oracle.DT_NP[dt]
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    if nd.kind != "V":
        return a.view(nd) < b.view(nd)
    wa, wb = a.view(np.uint64).reshape(-1, 2), b.view(np.uint64).reshape(-1, 2)
    ha, hb = wa[:, 1], wb[:, 1]
    if _signed(dt):
        ha, hb = ha.view(np.int64), hb.view(np.int64)
    return (ha < hb) | ((ha == hb) & (wa[:, 0] < wb[:, 0]))


SWAP_EDGE_PAIRS = ("+0,-0", "-0,+0", "nan,same nan", "nan,-nan", "1,nan", "nan,1", "inf,inf",
                   "-inf,inf", "subnormal,0")


def swap_edge_pairs(dt: int):
    """The edge lanes' (dst, cmp) as two (k, esz) byte arrays.  Float types,
    SWAP_EDGE_PAIRS in order (complex: the pair in both components): the +-0
    pairs and the same-NaN pair separate a compare of bits from one of
    values, the rest are the unordered and the infinite compares.  Integers:
    (min, max), (max, min), (min, min), (-1, 0)."""
    esz = esz_of(dt)
    if is_float(dt):
        ft = np.dtype(np.float32) if is_complex(dt) else oracle.DT_NP[dt]
        sub = np.finfo(ft).smallest_subnormal
        d = np.array([0.0, -0.0, np.nan, np.nan, 1.0, np.nan, np.inf, -np.inf, sub], ft)
        c = np.array([-0.0, 0.0, np.nan, -np.nan, np.nan, 1.0, np.inf, np.inf, 0.0], ft)
        if is_complex(dt):
            d, c = np.repeat(d, 2), np.repeat(c, 2)
        return d.view(np.uint8).reshape(-1, esz).copy(), c.view(np.uint8).reshape(-1, esz).copy()
    bits = 8 * esz
    lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if _signed(dt) else (0, (1 << bits) - 1)

    def enc(vals):
        return np.array([list((v % (1 << bits)).to_bytes(esz, "little")) for v in vals], np.uint8)
    pairs = [(lo, hi), (hi, lo), (lo, lo), (-1, 0)]
    return enc([p[0] for p in pairs]), enc([p[1] for p in pairs])


def swap_inputs(op: int, dt: int, n: int, rng):
    """dst, src, cmp of n elements (byte arrays) for a compare-table entry.

    The CSWAP family: per lane two values a != b of the type and a class
    drawn uniformly from {equal: cmp = dst = a; below: cmp = min, dst = max;
    above: cmp = max, dst = min} (complex, which has no order: equal, and
    differ twice), so every compare holds on 1/3 or 2/3 of the lanes and both
    outcomes of an ordered compare are reached on purpose.  src differs from
    dst in bits on every lane: a swap taken and a swap skipped always differ.
    MSWAP: uniform bytes.  The last 64 lanes hold swap_edge_pairs."""
    esz = esz_of(dt)
    if op == MSWAP:
        dst, src, cmp = (rng.integers(0, 256, (n, esz), dtype=np.uint8) for _ in range(3))
    else:
        a, b = _draw(dt, n, rng), _draw(dt, n, rng)
        same = values_equal(dt, a, b)
        while same.any():
            b[same] = _draw(dt, int(same.sum()), rng)
            same = values_equal(dt, a, b)
        cls = rng.integers(0, 3, n)[:, None]
        if is_complex(dt):
            lo, hi = a, b
        else:
            lt = _less(dt, a, b)[:, None]
            lo, hi = np.where(lt, a, b), np.where(lt, b, a)
        dst = np.where(cls == 0, a, np.where(cls == 1, hi, lo))
        cmp = np.where(cls == 0, a, np.where(cls == 1, lo, hi))
        src = _draw(dt, n, rng)
    ne = min(EDGE_LANES, n)
    ed, ec = swap_edge_pairs(dt)
    which = np.arange(ne) % ed.shape[0]
    dst[n - ne:], cmp[n - ne:] = ed[which], ec[which]
    if op != MSWAP:
        src[(src == dst).all(axis=1), 0] ^= 1
    return dst.reshape(-1), src.reshape(-1), cmp.reshape(-1)


# ----------------------------------------------------------- table cases --

class TableCase:
    """One binary-table call's operands in one arena: the outputs (dst, res)
    and the inputs.  `at`: operand name -> (start, bytes); `want`: the bytes
    dst must hold afterwards, compared byte for byte where `exact` (nothing
    is computed: the compare table, ATOMIC_READ), else through assert_same;
    `odd`: the operand off the others' alignment, or None."""

    def __init__(self, arena, at, want, exact, what, segs, path, odd):
        self.arena, self.at, self.want, self.exact = arena, at, want, exact
        self.what, self.segs, self.path, self.odd = what, segs, path, odd

    def view(self, buf, name):
        lo, nb = self.at[name]
        return buf[lo:lo + nb]

    def check(self, dt: int, got: np.ndarray) -> None:
        got = np.asarray(got)
        assert got.shape == self.arena.shape, self.what
        assert L.gaps_intact(got, self.segs), f"{self.what}: a gap lost its sentinel"
        for name in ("src", "cmp"):
            if name in self.at:
                assert np.array_equal(self.view(got, name), self.view(self.arena, name)), \
                    f"{self.what}: {name} changed"
        if "res" in self.at:        # a move: exact for every type
            assert np.array_equal(self.view(got, "res"), self.view(self.arena, "dst")), \
                f"{self.what}: res is not the old dst"
        if self.exact:
            assert np.array_equal(self.view(got, "dst"), self.want), f"{self.what}: dst"
        else:
            assert_same(dt, self.view(got, "dst").copy(), self.want, f"{self.what} dst")


def carve_table(dt, names, data, want, exact, path, k=0, what=""):
    """A TableCase for the operands `data` (name -> bytes; res, which has
    none, holds OUT_FILL) in `names` order on `path`."""
    esz = esz_of(dt)
    n = lanes(esz)
    assert n * esz == data["dst"].size
    offs, odd = table_layout(esz, path, names, k)
    segs, size = L.plan([n] * len(names), offs, esz)
    arena = np.full(size, L.SENTINEL, np.uint8)
    for name, (lo, nb) in zip(names, segs):
        arena[lo:lo + nb] = data[name] if name in data else OUT_FILL
    return TableCase(arena, dict(zip(names, segs)), want, exact,
                     f"{what} {path}" + (f" odd={odd}" if odd else ""), segs, path, odd)


def _on_paths(dt, names, data, want, exact, paths, turn, what):
    for path in paths_of(esz_of(dt)):
        if path in paths:
            yield carve_table(dt, names, data, want, exact, path, turn[path], what)
            turn[path] += 1


def write_cases(op, dts, rng, paths=PATHS):
    """Every case of lfa_atomic_write_async for one op: each type on each
    path, the odd operand rotating from case to case."""
    turn = dict.fromkeys(PATHS, 0)
    for dt in dts:
        d, s = inputs(SUM if op == WRITE else op, dt, 2, lanes(esz_of(dt)), rng)
        yield from ((dt, c) for c in _on_paths(
            dt, TABLE_OPERANDS["write"], {"dst": d, "src": s}, reference_write(op, dt, d, s),
            False, paths, turn, f"write op={op} dt={dt}"))


def readwrite_cases(op, dts, rng, paths=PATHS):
    """Every case of lfa_atomic_readwrite_async for one op.  ATOMIC_READ has
    no src: dst must come back as it was, byte for byte."""
    turn = dict.fromkeys(PATHS, 0)
    for dt in dts:
        n = lanes(esz_of(dt))
        if op == READ:
            (d,) = inputs(SUM, dt, 1, n, rng)
            names, data = TABLE_OPERANDS["read"], {"dst": d}
            want = reference_readwrite(op, dt, d, None)
        else:
            d, s = inputs(SUM if op == WRITE else op, dt, 2, n, rng)
            names, data = TABLE_OPERANDS["readwrite"], {"dst": d, "src": s}
            want = reference_readwrite(op, dt, d, s)
        yield from ((dt, c) for c in _on_paths(dt, names, data, want, op == READ, paths, turn,
                                               f"readwrite op={op} dt={dt}"))


def swap_cases(op, dts, rng, paths=PATHS):
    """Every case of lfa_atomic_swap_async for one op."""
    turn = dict.fromkeys(PATHS, 0)
    for dt in dts:
        d, s, c = swap_inputs(op, dt, lanes(esz_of(dt)), rng)
        yield from ((dt, case) for case in _on_paths(
            dt, TABLE_OPERANDS["swap"], {"dst": d, "src": s, "cmp": c},
            reference_swap(op, dt, d, s, c), True, paths, turn, f"swap op={op} dt={dt}"))


def operands_of(table: str, op: int):
    return TABLE_OPERANDS["read" if table == "readwrite" and op == READ else table]


def assert_every_operand_was_odd(table: str, op: int, cases) -> None:
    """Over `cases` ((dt, TableCase) of one op of a table) every operand that
    can take the odd offset on a path did so at least once; a fortiori over
    the table."""
    for path, cands in ODD.items():
        seen = {c.odd for _, c in cases if c.path == path}
        assert seen == {o for o in cands if o in operands_of(table, op)}, (table, op, path, seen)


# ----------------------------------------------------- large-size forms ----
# The forms launch_write and launch_tree_body only take from 32 or 192 MiB per
# operand (lfa_split.h: lfa_form_write / lfa_form_tree), run at lanes()
# through the lfa__write_as and lfa__tree_as entries, which choose the form as if the body
# were `as_bytes` bytes and leave everything else to the real size
# (tests/test_sweep_forms_gpu.py).  The model below is written from the
# launchers' table of forms, not from the C functions: tests/test_split_cpu.py
# holds tools/split_host_check.cpp's output to it.

MIB = 1 << 20
WRITE_FORMS = ("combine_lds sc1", "combine_lds_taper sc1", "combine_lds nt")    # enum order
TREE_FORMS = {1: "chunk1 nt", 2: "chunk2 nt", 3: "lds", 11: "chunk2 sc1", 25: "put body"}
SMALL_FORMS = {"combine_lds sc1", "chunk2 sc1", "chunk2 sc1 +cap", "put body"}


def model_write_form(nbytes: int, mapped: bool = False) -> str:
    """launch_write: the tapered grid from 32 MiB, nt stores (drained) from
    192 MiB; host-mapped operands keep the small form at every size."""
    if mapped or nbytes < 32 * MIB:
        return "combine_lds sc1"
    return "combine_lds_taper sc1" if nbytes < 192 * MIB else "combine_lds nt"


def leaves_of(nsrc: int) -> int:
    return 1 << (nsrc.bit_length() - 1)


def model_tree_form(nbytes: int, nsrc: int, esz: int) -> str:
    """launch_tree_body: from 192 MiB of output the LDS form at 2 inputs,
    chunk U=1 at 3..8, chunk U=2 above, all with nt stores; below, the
    put body at 8..15 inputs of 4-byte or wider elements, else chunk U=2
    write-through, with the 41 KiB LDS cap at 3..8 inputs."""
    if nbytes >= 192 * MIB:
        return "lds" if nsrc == 2 else "chunk1 nt" if nsrc <= 8 else "chunk2 nt"
    if leaves_of(nsrc) == 8 and esz >= 4:
        return "put body"
    return "chunk2 sc1 +cap" if 3 <= nsrc <= 8 else "chunk2 sc1"


def model_taper(nvec: int, div: int, hv: int = 1024, tv: int = 256):
    """lfa_split_taper: (head workgroups, whole tail workgroups, vectors in
    the last, partial one)."""
    split = (nvec - nvec // div) // hv * hv
    return split // hv, (nvec - split) // tv, (nvec - split) % tv


FORM_PATHS = ("vec", "head")        # the paths with a vector body
WRITE_AS = (("combine_lds_taper sc1", 32 * MIB), ("combine_lds nt", 192 * MIB))
TREE_AS = 192 * MIB
# the large-only tree instantiation each fan-in of TREE_NSRC reaches
TREE_AS_FORMS = {2: "lds", 3: "chunk1 nt", 5: "chunk1 nt", 8: "chunk1 nt", 9: "chunk2 nt",
                 17: "chunk2 nt", 32: "chunk2 nt"}


def write_form_cases(op, dts, rng):
    """(form, as_bytes, dt, TableCase): every type of the op on the vec and
    head paths, under the tapered and under the nt-drained write body."""
    for form, as_bytes in WRITE_AS:
        for dt, case in write_cases(op, dts, rng, FORM_PATHS):
            yield form, as_bytes, dt, case


def tree_form_cases(op, dt, rng):
    """(form, as_bytes, Case): each fan-in of TREE_NSRC on the vec path, and
    with the output aliasing the highest input and input 0.  (On the head
    path the tree takes the element kernel for the whole buffer.)"""
    esz = esz_of(dt)
    for nsrc in TREE_NSRC:
        data = inputs(op, dt, nsrc, lanes(esz), rng)
        want = reference(op, dt, data)
        for alias in (None,) + TREE_ALIAS:
            yield TREE_AS_FORMS[nsrc], TREE_AS, carve(
                dt, data, want, "vec", alias=alias,
                what=f"tree as {TREE_AS_FORMS[nsrc]} op={op} dt={dt} nsrc={nsrc} out is {alias}")


def n_tree_form_cases(op) -> int:
    return len(dts_of(op)) * len(TREE_NSRC) * (1 + len(TREE_ALIAS))
