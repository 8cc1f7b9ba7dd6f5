"""The oracle sweep's cases and inputs: no GPU, no product code.

tests/test_sweep_gpu.py runs every (op, datatype) pair through every tree,
tree-put and list-form kernel instantiation liblfa.so holds,
tests/test_sweep_tables_gpu.py every entry of the write, fetch and compare
tables through its own kernels, tests/test_sweep_forms_gpu.py every form the
write, tree and fetch launchers only take at large sizes, tests/test_sweep_oneshot_gpu.py
every one-shot kernel, one rank at a time (the last parts of this module);
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


def carve_table(dt, names, data, want, exact, path, k=0, what="", count=lanes):
    """A TableCase for the operands `data` (name -> bytes; res, which has
    none, holds OUT_FILL) in `names` order on `path`; count(esz) elements."""
    esz = esz_of(dt)
    n = count(esz)
    assert n * esz == data["dst"].size
    offs, odd = table_layout(esz, path, names, k)
    segs, size = L.plan([n] * len(names), offs, esz)
    arena = np.full(size, L.SENTINEL, np.uint8)
    for name, (lo, nb) in zip(names, segs):
        arena[lo:lo + nb] = data[name] if name in data else OUT_FILL
    return TableCase(arena, dict(zip(names, segs)), want, exact,
                     f"{what} {path}" + (f" odd={odd}" if odd else ""), segs, path, odd)


def _on_paths(dt, names, data, want, exact, paths, turn, what, count=lanes):
    for path in paths_of(esz_of(dt)):
        if path in paths:
            yield carve_table(dt, names, data, want, exact, path, turn[path], what, count)
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


def readwrite_cases(op, dts, rng, paths=PATHS, count=lanes):
    """Every case of lfa_atomic_readwrite_async for one op.  ATOMIC_READ has
    no src: dst must come back as it was, byte for byte.  count(esz): the
    elements per operand."""
    turn = dict.fromkeys(PATHS, 0)
    for dt in dts:
        n = count(esz_of(dt))
        if op == READ:
            (d,) = inputs(SUM, dt, 1, n, rng)
            names, data = TABLE_OPERANDS["read"], {"dst": d}
            want = reference_readwrite(op, dt, d, None)
        else:
            d, s = inputs(SUM if op == WRITE else op, dt, 2, n, rng)
            names, data = TABLE_OPERANDS["readwrite"], {"dst": d, "src": s}
            want = reference_readwrite(op, dt, d, s)
        yield from ((dt, c) for c in _on_paths(dt, names, data, want, op == READ, paths, turn,
                                               f"readwrite op={op} dt={dt}", count))


def swap_cases(op, dts, rng, paths=PATHS, count=lanes):
    """Every case of lfa_atomic_swap_async for one op; count(esz): the
    elements per operand."""
    turn = dict.fromkeys(PATHS, 0)
    for dt in dts:
        d, s, c = swap_inputs(op, dt, count(esz_of(dt)), rng)
        yield from ((dt, case) for case in _on_paths(
            dt, TABLE_OPERANDS["swap"], {"dst": d, "src": s, "cmp": c},
            reference_swap(op, dt, d, s, c), True, paths, turn, f"swap op={op} dt={dt}",
            count))


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


# The forms launch_fetch only takes from 64 or 192 MiB per operand
# (lfa_split.h: lfa_form_fetch), through the lfa__readwrite_as and lfa__swap_as
# entries.  nin: the functor's inputs: 1 ATOMIC_READ (dst), 2 the other
# readwrite ops (dst, src), 3 the compare table (dst, src, cmp).

FETCH_FORMS = ("fetch_lds sc1", "fetch_lds_taper sc1", "fetch_lds_taper nt")     # enum order
FETCH_AS = (("fetch_lds_taper nt", 192 * MIB), ("fetch_lds_taper sc1", 64 * MIB))
# the form cases of the two tables: (pairs on the vec path + on the head
# path) per forced form; 24 of the 145 readwrite pairs are 16-byte types (2 of
# them ATOMIC_READ's, which has no tapered write-through form), 14 of the 84
# compare pairs
N_RW_FORM_CASES = (145 + 121) + (132 + 110)
N_SWAP_FORM_CASES = 84 + 70


def model_fetch_form(nbytes: int, nin: int) -> str:
    """launch_fetch: below 64 MiB fetch_lds with write-through stores; from
    64 MiB the tapered kernel with write-through stores for two-input
    functors only; from 192 MiB the tapered kernel with nt stores for all."""
    if nbytes >= 192 * MIB:
        return "fetch_lds_taper nt"
    return "fetch_lds_taper sc1" if nin == 2 and nbytes >= 64 * MIB else "fetch_lds sc1"


def fetch_nin(table: str, op: int) -> int:
    return 3 if table == "swap" else 1 if op == READ else 2


def fetch_lanes(esz: int) -> int:
    """The count of the fetch form cases.  launch_fetch tapers the last 1/4 in
    256-vector workgroups behind 1024-vector head workgroups, where lanes()
    leaves ONE head workgroup; this gives 3172..3174 vectors: two whole head
    workgroups, four whole tail workgroups, a last one of 100..102 vectors
    (a whole wave and a partial one) and, below 16 bytes, an element tail.
    One element past a whole number of vectors, not lanes()'s three: behind
    the head path's 16 / esz - 1 head elements three more leave no tail at 4
    bytes, one leaves two elements at 1, 2 and 4 bytes.  (At 8 bytes no count
    has a tail on both paths: the one head element takes it.)"""
    return (48 * 1024 + 16 * 101) // esz + 1


def readwrite_form_cases(op, dts, rng):
    """(form, as_bytes, dt, TableCase): every type of the op on the vec and
    head paths under the tapered nt-store fetch body and, except ATOMIC_READ
    (one input: the launcher never gives it that form), under the tapered
    write-through one."""
    for form, as_bytes in FETCH_AS:
        if model_fetch_form(as_bytes, fetch_nin("readwrite", op)) != form:
            assert op == READ and form == "fetch_lds_taper sc1"
            continue
        for dt, case in readwrite_cases(op, dts, rng, FORM_PATHS, fetch_lanes):
            yield form, as_bytes, dt, case


def swap_form_cases(op, dts, rng):
    """(form, as_bytes, dt, TableCase): every type of the op on the vec and
    head paths under the tapered nt-store compare body."""
    form, as_bytes = FETCH_AS[0]
    assert model_fetch_form(as_bytes, fetch_nin("swap", op)) == form
    for dt, case in swap_cases(op, dts, rng, FORM_PATHS, fetch_lanes):
        yield form, as_bytes, dt, case


def n_fetch_form_cases(table: str, op: int, dts) -> int:
    forms = sum(model_fetch_form(a, fetch_nin(table, op)) == f for f, a in FETCH_AS)
    return (forms if table == "readwrite" else 1) * n_table_cases(dts, FORM_PATHS)


# ------------------------------------------------------------- one-shot ----
# The one-shot kernels (lfa_k_oneshot.hpp): oneshot_reduce<OP, T, 1|2|4|8> and
# oneshot_ll<OP, T, 2|4|8>, run one rank at a time on one stream
# (tests/test_sweep_oneshot_gpu.py).  Rank r's kernel waits only on its own
# workspace, so with the flags posted beforehand it never has to wait, and
# what it pushed and posted can be read back.  Below: a model of the layout in
# lfa_signal.h and launch_oneshot (tests/test_sweep_cpu.py holds the constants
# to the header's text), the case builder, the protocol (os_run) over a
# `dev` that holds the buffers, and OsEmu, a numpy dev that emulates push,
# post, wait and reduce, so the protocol is proved before it meets a kernel.

OS_ALL, OS_SCATTER = -1, -2         # struct lfa_oneshot's mode; >= 0: reduce to that root
FLAG, LL = "flag", "ll"             # the kernels; lfa__oneshot_as's ll argument below
OS_LL_ARG = {FLAG: 0, LL: 1}
SIG_MAX, SIG_AREA, SIG_OS_OFF, SIG_OS_CHUNKS, OS_MAX_RANKS = 32, 1 << 20, 256, 128, 8
LL_BYTES = 16 << 10
LL_SLOT, LL_PARITY, LL_OFF = 2 * LL_BYTES, 8 * 2 * LL_BYTES, 64 << 10
OS_MIN_CHUNK = 4096
SIG_NONE = 0xFFFFFFFFFFFFFFFF
WS_FILL = 0xA5                      # a workspace byte nothing wrote
LL_JUNK = 0x5EED1E55                # the data word of an LL pair nothing pushed
OS_TIMEOUT_US = 2_000_000           # a guard no correct run reaches
OS_NLEAF = {FLAG: (1, 2, 4, 8), LL: (2, 4, 8)}
N_OS_INSTANCES = 133 * (4 + 3)      # the instantiations launch_oneshot chooses among


def os_parts(mode: int, n: int, count: int, esz: int):
    """(soff, slen) in bytes: the range of every rank's input that member k
    reduces (launch_oneshot; SCATTER is lfa_coll_block's partition)."""
    if mode == OS_SCATTER:
        base, extra = divmod(count, n)
        return ([(k * base + min(k, extra)) * esz for k in range(n)],
                [(base + (k < extra)) * esz for k in range(n)])
    return [0] * n, [count * esz if mode in (OS_ALL, k) else 0 for k in range(n)]


def os_grid(kernel: str, most: int):
    """(chunk, workgroups) for a largest part of `most` bytes.  Flagged: at
    most LFA_SIG_OS_CHUNKS chunks, a multiple of 16, never below 4096.  LL:
    16 bytes per lane, 256 lanes per workgroup (chunk is None)."""
    if kernel == LL:
        return None, -(-(-(-most // 16)) // 256)
    chunk = max((-(-most // SIG_OS_CHUNKS) + 15) // 16 * 16, OS_MIN_CHUNK)
    return chunk, -(-most // chunk)


def os_offsets(esz: int, path: str, flip: int = 0):
    """(send, result) byte offsets past a 16-byte boundary.  vec: both
    aligned; head: both one element on; elem: one of them one element on
    (which: flip); bytes: one of them one byte off the element."""
    assert path in paths_of(esz), (esz, path)
    if path == "vec":
        return 0, 0
    if path == "head":
        return esz, esz
    d = esz if path == "elem" else 1
    return (0, d) if flip % 2 == 0 else (d, 0)


def ll_pack(part: np.ndarray, flag: int, fill: int = 0) -> np.ndarray:
    """A part as the LL kernel pushes it: zero-padded to 16 bytes, every 4
    bytes followed by the flag word."""
    pad = np.full(-(-part.size // 16) * 16, fill, np.uint8)
    pad[:part.size] = part
    w = np.empty((pad.size // 4, 2), np.uint32)
    w[:, 0], w[:, 1] = pad.view(np.uint32), flag
    return w.reshape(-1).view(np.uint8)


def ll_unpack(words: np.ndarray):
    """(data bytes, flag words) of LL pairs."""
    w = np.ascontiguousarray(words).view(np.uint32).reshape(-1, 2)
    return np.ascontiguousarray(w[:, 0]).view(np.uint8), w[:, 1].copy()


class OsCase:
    """One one-shot operation of n ranks: every rank's send and result carved
    from one arena (`sends[r]`, `results[r]`: (start, bytes), or None for a
    rank without a result), the smallest legal workspaces, and `want[r]`: the
    bytes rank r's result must hold."""

    def __init__(self, op, dt, n, mode, count, kernel, path, epoch, data, flip=0, done=False,
                 ll=None, what=""):
        esz = esz_of(dt)
        assert 1 <= n <= OS_MAX_RANKS and all(x.size == count * esz for x in data)
        self.op, self.dt, self.n, self.mode, self.count = op, dt, n, mode, count
        self.kernel, self.path, self.epoch, self.done = kernel, path, epoch & 0xFFFFFFFF, done
        self.ll = OS_LL_ARG[kernel] if ll is None else ll
        self.soff, self.slen = os_parts(mode, n, count, esz)
        self.most = max(self.slen)
        assert kernel == FLAG or (n > 1 and self.most <= LL_BYTES and mode < 0)
        self.chunk, self.grid = os_grid(kernel, self.most)
        self.nleaf = leaves_of(n)
        # lfa_signal.h: a slot is the largest part rounded up to 256; the odd
        # epochs' slots lie parity_off above the even ones; then the flag area
        self.slot_bytes = -(-self.most // 256) * 256
        self.parity_off = n * self.slot_bytes
        self.flag_off = 2 * self.parity_off
        self.ws_bytes = self.flag_off + SIG_AREA if n > 1 else 0
        self.flag = (2 * self.epoch + 1) & 0xFFFFFFFF
        s_off, r_off = os_offsets(esz, path, flip)
        has = [r for r in range(n) if self.slen[r]]
        self.segs, size = L.plan([count * esz] * n + [self.slen[r] for r in has],
                                 [s_off] * n + [r_off] * len(has), 1)
        self.sends = self.segs[:n]
        self.results = [None] * n
        for r, seg in zip(has, self.segs[n:]):
            self.results[r] = seg
        self.arena = np.full(size, L.SENTINEL, np.uint8)
        for (lo, nb), x in zip(self.sends, data):
            self.arena[lo:lo + nb] = x
        for r in has:
            lo, nb = self.results[r]
            self.arena[lo:lo + nb] = OUT_FILL
        full = data[0] if n == 1 else reference(op, dt, data)      # one rank: a copy
        self.want = [full[self.soff[r]:self.soff[r] + self.slen[r]] if self.slen[r] else None
                     for r in range(n)]
        # what launch_oneshot derives from the addresses (the arena is 16-B aligned)
        self.unal = bool(s_off % esz or (has and r_off % esz))
        mis = any((s_off + o) % 16 for o in self.soff) or bool(has and r_off % 16)
        self.vec = not mis and (kernel == LL or not self.unal)
        self.what = what or (f"oneshot {kernel} op={op} dt={dt} n={n} mode={mode} count={count} "
                             f"{path} epoch={self.epoch:#x}")

    # ---- where things live in member j's workspace (bytes) ----
    def slot_at(self, k: int) -> int:
        return (self.epoch & 1) * self.parity_off + k * self.slot_bytes

    def flag_at(self, b: int, k: int) -> int:
        return self.flag_off + SIG_OS_OFF + 4 * (b * SIG_MAX + k)

    def ll_slot_at(self, k: int) -> int:
        return self.flag_off + LL_OFF + (self.epoch & 1) * LL_PARITY + k * LL_SLOT

    def send_part(self, r: int, k: int) -> np.ndarray:
        """The bytes of rank r's input that member k reduces."""
        lo = self.sends[r][0] + self.soff[k]
        return self.arena[lo:lo + self.slen[k]]

    def preposted(self, ws: np.ndarray) -> None:
        """Fill the members' workspaces (back to back in ws) as before the
        first launch: WS_FILL, and the flags every wait of this epoch accepts
        (flagged: every one-shot flag word epoch + 1, which a kernel's own
        post of `epoch` stays distinguishable from; LL: every pair of this
        parity's slots {junk, 2·epoch + 1})."""
        ws[:] = WS_FILL
        for j in range(self.n if self.ws_bytes else 0):
            m = ws[j * self.ws_bytes:(j + 1) * self.ws_bytes]
            if self.kernel == FLAG:
                lo = self.flag_at(0, 0)
                m[lo:lo + 4 * SIG_OS_CHUNKS * SIG_MAX].view(np.uint32)[:] = \
                    (self.epoch + 1) & 0xFFFFFFFF
            else:
                lo = self.ll_slot_at(0)
                w = m[lo:lo + LL_PARITY].view(np.uint32).reshape(-1, 2)
                w[:, 0], w[:, 1] = LL_JUNK, self.flag

    def windows(self):
        """[(start in the back-to-back workspaces, expected bytes, what)]:
        everything one pass of all ranks writes into the workspaces."""
        out = []
        for j in range(self.n if self.ws_bytes else 0):
            base = j * self.ws_bytes
            for r in range(self.n):
                if r == j or not self.slen[j]:
                    continue
                part = self.send_part(r, j)
                if self.kernel == FLAG:
                    out.append((base + self.slot_at(r), part.copy(), f"slot {r} at member {j}"))
                else:
                    out.append((base + self.ll_slot_at(r), ll_pack(part, self.flag),
                                f"LL slot {r} at member {j}"))
            if self.kernel == FLAG:
                rows = np.full((self.grid, SIG_MAX), (self.epoch + 1) & 0xFFFFFFFF, np.uint32)
                for r in range(self.n):
                    if r != j:
                        rows[:, r] = self.epoch
                out.append((base + self.flag_at(0, 0), rows.reshape(-1).view(np.uint8),
                            f"flag rows of member {j}"))
        return out

    def check(self, got: np.ndarray) -> None:
        got = np.asarray(got)
        assert got.shape == self.arena.shape, self.what
        assert L.gaps_intact(got, self.segs), f"{self.what}: a gap lost its sentinel"
        for r, (lo, nb) in enumerate(self.sends):
            assert np.array_equal(got[lo:lo + nb], self.arena[lo:lo + nb]), \
                f"{self.what}: input {r} changed"
        for r, seg in enumerate(self.results):
            if seg is not None:
                lo, nb = seg
                assert_same(self.dt, got[lo:lo + nb].copy(), self.want[r],
                            f"{self.what} rank {r}")


def os_run(case: OsCase, dev) -> None:
    """The protocol.  dev.load(case) uploads the arena and prepares the
    workspaces as OsCase.preposted does; dev.launch(case, r, done_val)
    launches rank r's kernel, synchronises and returns (status word, done
    word, done counter) (the last two None without done_val); dev.gather
    downloads ranges of the workspaces, dev.untouched says whether everything
    outside them still holds what load left; dev.refill puts OUT_FILL back
    into the results; dev.arena downloads the arena."""
    dev.load(case)
    for p in (1, 2):
        # pass 1 pushes and posts (its results are meaningless: early ranks
        # read slots not pushed yet); pass 2, same epoch, reduces what is there
        for r in range(case.n):
            val = (0x0D0E000000000000 | p << 8 | r) if case.done else 0
            status, word, ctr = dev.launch(case, r, val)
            assert status == SIG_NONE, f"{case.what}: rank {r} pass {p} timed out ({status:#x})"
            if case.done:   # the counter reads 0 again: the next launch reuses it
                assert (word, ctr) == (val, 0), f"{case.what}: rank {r} pass {p} done {word:#x} {ctr}"
        if p == 2:
            break
        wins = case.windows()
        ranges = [(lo, b.size) for lo, b, _ in wins]
        got = dev.gather(ranges)
        at = 0
        for lo, want, what in wins:
            g = got[at:at + want.size]
            at += want.size
            if not np.array_equal(g, want):
                i = int(np.nonzero(g != want)[0][0])
                raise AssertionError(f"{case.what}: {what} differs from byte {i}: got "
                                     f"{g[i:i + 8].tolist()} want {want[i:i + 8].tolist()}")
        assert dev.untouched(ranges), \
            f"{case.what}: a workspace byte outside the expected pushes and posts changed"
        dev.refill(case)
    case.check(dev.arena())


class OsEmu:
    """A numpy dev: each launch pushes, posts, waits and reduces as the
    kernels' comments say, through OsCase's layout.  `fault`: one of
    OS_FAULTS, to show that os_run sees it."""

    def __init__(self, fault=None):
        self.fault = fault

    def load(self, c):
        self.a = c.arena.copy()
        self.ws = np.empty(c.n * c.ws_bytes, np.uint8)
        c.preposted(self.ws)
        self.base = self.ws.copy()

    def _part(self, c, r, k, nb=None):
        off = c.soff[r if self.fault == "soff_rank" and c.kernel == FLAG else k]
        lo = c.sends[r][0] + off
        return self.a[lo:lo + (c.slen[k] if nb is None else nb)]

    def launch(self, c, r, done_val):
        status, W = SIG_NONE, c.ws_bytes
        mine = self.ws[r * W:(r + 1) * W]
        post = (c.epoch - (self.fault == "post_minus_1")) & 0xFFFFFFFF
        ins = []
        for k in range(c.n):
            if k == r:
                ins.append(self._part(c, r, r).copy())
                continue
            peer = self.ws[k * W:(k + 1) * W]
            if c.kernel == FLAG:
                lo = c.slot_at(r)
                peer[lo:lo + c.slen[k]] = self._part(c, r, k)
                for b in range(c.grid):
                    peer[c.flag_at(b, r):c.flag_at(b, r) + 4].view(np.uint32)[0] = post
                    w = int(mine[c.flag_at(b, k):c.flag_at(b, k) + 4].view(np.uint32)[0])
                    if (w - c.epoch) & 0x80000000:      # the wait's signed compare
                        status = 1
                lo = c.slot_at(k)
                ins.append(mine[lo:lo + c.slen[r]].copy())
            else:
                if c.slen[k]:
                    words = ll_pack(self._part(c, r, k), c.flag,
                                    0x5A if self.fault == "no_zero_fill" else 0)
                    lo = c.ll_slot_at(r)
                    peer[lo:lo + words.size] = words
                lo = c.ll_slot_at(k)
                data, flags = ll_unpack(mine[lo:lo + 2 * (-(-c.slen[r] // 16) * 16)])
                if (flags != c.flag).any():
                    status = 1
                ins.append(data[:c.slen[r]].copy())
        if c.slen[r] and status == SIG_NONE:
            if self.fault == "leaf0_for_7" and c.n == 8:
                ins[7] = ins[0]
            if self.fault == "swap_node" and c.n > c.nleaf:
                ins[0], ins[1] = ins[1], ins[0]
            out = ins[0] if c.n == 1 else reference(c.op, c.dt, ins)
            lo, nb = c.results[r]
            if self.fault == "vhi_hi" and c.kernel == FLAG and c.vec:
                nb -= nb % 16
            self.a[lo:lo + nb] = out[:nb]
        return status, (done_val if done_val else None), (0 if done_val else None)

    def gather(self, ranges):
        return np.concatenate([self.ws[lo:lo + nb] for lo, nb in ranges] or
                              [np.zeros(0, np.uint8)])

    def untouched(self, ranges):
        d = self.ws != self.base
        for lo, nb in ranges:
            d[lo:lo + nb] = False
        return not d.any()

    def refill(self, c):
        for seg in c.results:
            if seg is not None:
                self.a[seg[0]:seg[0] + seg[1]] = OUT_FILL

    def arena(self):
        return self.a


OS_FAULTS = ("swap_node", "leaf0_for_7", "vhi_hi", "soff_rank", "post_minus_1", "no_zero_fill")

# ---- the cases ----
# (ranks, mode) per pair: flagged (NLEAF 1, 2, 2, 4, 8; scatter; reduce to a
# root that is not rank 0) and LL
OS_ROW_FLAG = ((1, OS_ALL), (2, OS_ALL), (3, OS_ALL), (5, OS_ALL), (8, OS_ALL),
               (3, OS_SCATTER), (8, OS_SCATTER), (2, 1), (5, 3))
OS_ROW_LL = ((2, OS_ALL), (3, OS_ALL), (5, OS_ALL), (8, OS_ALL), (3, OS_SCATTER), (8, OS_SCATTER))
OS_ROWS = {FLAG: OS_ROW_FLAG, LL: OS_ROW_LL}
OS_FOLD_N = (4, 6, 7)               # tree_leaves' folding at the remaining rank counts
OS_EPOCHS = (1, 2, 0x7FFFFFFF, 0xFFFFFFFF)
OS_EPOCH_N = {FLAG: (1, 2, 5, 8), LL: (2, 5, 8)}
# largest part in bytes before the odd elements: 2 whole 4-KiB workgroups and
# 80 bytes (flagged: a partial chunk with a vector body and a tail); 9 KiB (LL)
OS_PART = {FLAG: 2 * 4096 + 80, LL: 9 << 10}
OS_ODD = 3
OS_BIG_PART = 128 * 4096 + 4096 + 48        # chunk > 4096: 4144, 128 workgroups
N_OS_PAIR_CASES = len(OS_ROW_FLAG) + len(OS_ROW_LL)                 # 15 per pair
# per op: folding, epochs, size edges, completion word
N_OS_OP_CASES = 3 + 4 * (4 + 3) + 11 + 4                            # 46
N_OS_CASES = 133 * 15 + 10 * 46                                     # 2455


def os_count(kernel: str, mode: int, n: int, esz: int) -> int:
    """Elements for the rows' shape: the largest part is OS_PART[kernel]
    bytes plus OS_ODD elements (SCATTER: the last rank's is one shorter)."""
    per = OS_PART[kernel] // esz + OS_ODD
    return n * per - 1 if mode == OS_SCATTER else per


def os_dt(op: int, salt: int) -> int:
    """One datatype of the op, another one for another salt."""
    dts = dts_of(op)
    return dts[(op + salt) % len(dts)]


def _os_case(op, dt, n, mode, count, kernel, path, epoch, rng, **kw):
    return OsCase(op, dt, n, mode, count, kernel, path, epoch,
                  inputs(op, dt, n, count, rng), **kw)


def os_pair_cases(op, dt, rng):
    """The 15 cases every pair runs.  The path rotates with the row and with
    the pair's index in its op, so every pair meets every path its element
    size has on both kernels and every op meets every (path, NLEAF); the
    epoch's parity alternates from case to case."""
    esz = esz_of(dt)
    paths, i = paths_of(esz), dts_of(op).index(dt)
    for kernel in (FLAG, LL):
        for ci, (n, mode) in enumerate(OS_ROWS[kernel]):
            turn = ci + i
            yield _os_case(op, dt, n, mode, os_count(kernel, mode, n, esz), kernel,
                           paths[turn % len(paths)], 10 + turn, rng, flip=turn // len(paths))


def os_op_cases(op, rng):
    """The 46 cases every op runs on one datatype each: the non-power-of-two
    folding at 4, 6 and 7 ranks; both parities and the epochs around 2^31 and
    2^32 per (kernel, NLEAF); the size edges; the completion word."""
    turn = 0

    def case(dt, n, mode, count, kernel, path="vec", epoch=None, **kw):
        nonlocal turn
        turn += 1
        return _os_case(op, dt, n, mode, count, kernel, path,
                        20 + turn if epoch is None else epoch, rng, **kw)
    for n in OS_FOLD_N:
        dt = os_dt(op, n)
        yield case(dt, n, OS_ALL, os_count(FLAG, OS_ALL, n, esz_of(dt)), FLAG,
                   paths_of(esz_of(dt))[n % len(paths_of(esz_of(dt)))])
    for ki, kernel in enumerate((FLAG, LL)):
        for n in OS_EPOCH_N[kernel]:
            dt = os_dt(op, 10 * ki + n)
            for epoch in OS_EPOCHS:
                yield case(dt, n, OS_ALL, os_count(kernel, OS_ALL, n, esz_of(dt)), kernel,
                           epoch=epoch)
    dt = os_dt(op, 7)
    esz = esz_of(dt)
    for kernel, n in ((FLAG, 1), (FLAG, 3), (LL, 3)):               # one element
        yield case(dt, n, OS_ALL, 1, kernel)
    for kernel in (FLAG, LL):       # empty blocks: the last rank has no result
        for n in (3, 8):
            yield case(dt, n, OS_SCATTER, n - 1, kernel)
    yield case(dt, 2, OS_ALL, LL_BYTES // esz, LL)                  # the largest LL part
    yield case(dt, 2, OS_ALL, LL_BYTES // esz + 1, FLAG)            # one element above it
    for n in (2, 3):
        yield case(dt, n, OS_ALL, OS_BIG_PART // esz, FLAG)
    for ki, kernel in enumerate((FLAG, LL)):                        # completion word
        dt = os_dt(op, 3 + ki)
        for count in (256 // esz_of(dt) + OS_ODD, os_count(kernel, OS_ALL, 2, esz_of(dt))):
            yield case(dt, 2, OS_ALL, count, kernel, done=True)


def os_cases(op, rng):
    for dt in dts_of(op):
        yield from os_pair_cases(op, dt, rng)
    yield from os_op_cases(op, rng)
