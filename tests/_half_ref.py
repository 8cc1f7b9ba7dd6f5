"""Independent reference for FI_FLOAT16 / FI_BFLOAT16 reduction (no product
code): numpy float16 arithmetic for fp16, float32 arithmetic plus the
round-to-nearest-even shift for bf16, torch CPU as a second opinion on
SUM / PROD, `np.where(d > s, s, d)` on the widened values for MIN / MAX, and
a restatement of prov/coll's association order.

Everything works on uint16 bit patterns.  Comparison rule (tests/_cmp.py's,
for 16-bit lanes): the NaN class must match, every other lane is bit-exact.
"""
import functools

import numpy as np

FLOAT16, BFLOAT16 = 16, 17
MIN, MAX, SUM, PROD, LOR, LAND, BOR, BAND, LXOR, BXOR, READ, WRITE = range(12)
OPS = (MIN, MAX, SUM, PROD, LOR, LAND, LXOR, WRITE)   # the float column's write rows
NAMES = {FLOAT16: "fp16", BFLOAT16: "bf16"}
ONE = {FLOAT16: 0x3C00, BFLOAT16: 0x3F80}
INF = {FLOAT16: 0x7C00, BFLOAT16: 0x7F80}


def u16(a) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint16)


def widen(dt: int, u: np.ndarray) -> np.ndarray:
    u = u16(u)
    if dt == FLOAT16:
        return u.view(np.float16).astype(np.float32)
    return (u.astype(np.uint32) << 16).view(np.float32)


def narrow(dt: int, f: np.ndarray) -> np.ndarray:
    f = np.ascontiguousarray(f, dtype=np.float32)
    if dt == FLOAT16:
        with np.errstate(over="ignore", invalid="ignore"):
            return f.astype(np.float16).view(np.uint16)
    u = f.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    r[np.isnan(f)] = 0x7FC0
    return r


def isnan(dt: int, u: np.ndarray) -> np.ndarray:
    return (u16(u) & 0x7FFF) > INF[dt]


def from_float(dt: int, f) -> np.ndarray:
    return narrow(dt, np.asarray(f, dtype=np.float32))


def step(dt: int, op: int, d: np.ndarray, s: np.ndarray) -> np.ndarray:
    """One pairwise step d OP s."""
    d, s = u16(d), u16(s)
    wd, ws = widen(dt, d), widen(dt, s)
    with np.errstate(all="ignore"):
        if op == MIN:
            return np.where(wd > ws, s, d)
        if op == MAX:
            return np.where(wd < ws, s, d)
        if op in (SUM, PROD):
            if dt == FLOAT16:      # numpy's own float16 arithmetic
                a, b = d.view(np.float16), s.view(np.float16)
                return (a + b if op == SUM else a * b).view(np.uint16)
            return narrow(dt, wd + ws if op == SUM else wd * ws)
        td, ts = wd != 0, ws != 0
        if op == LOR:
            t = td | ts
        elif op == LAND:
            t = td & ts
        elif op == LXOR:
            t = td ^ ts
        elif op == WRITE:
            return s.copy()
        else:
            raise ValueError(op)
        return np.where(t, np.uint16(ONE[dt]), np.uint16(0)).astype(np.uint16)


def step_torch(dt: int, op: int, d: np.ndarray, s: np.ndarray) -> np.ndarray:
    """SUM / PROD as torch CPU computes them in the 16-bit type."""
    import torch
    tt = torch.float16 if dt == FLOAT16 else torch.bfloat16
    a = torch.from_numpy(u16(d).view(np.int16).copy()).view(tt)
    b = torch.from_numpy(u16(s).view(np.int16).copy()).view(tt)
    r = a + b if op == SUM else a * b
    return r.view(torch.int16).numpy().view(np.uint16)


def tree_with(fn, inputs):
    """prov/coll's association (lfa_host.cpp's comment): leaves are
    in[2k+1] OP in[2k] for k < rem, then single inputs; partials then merge
    pairwise, higher OP lower, level by level."""
    n = len(inputs)
    pof2 = 1
    while pof2 * 2 <= n:
        pof2 *= 2
    rem = n - pof2
    parts = [fn(inputs[2 * k + 1], inputs[2 * k]) if k < rem else inputs[k + rem]
             for k in range(pof2)]
    while len(parts) > 1:
        parts = [fn(parts[2 * j + 1], parts[2 * j]) for j in range(len(parts) // 2)]
    return parts[0]


def tree(dt: int, op: int, inputs) -> np.ndarray:
    return u16(tree_with(lambda d, s: step(dt, op, d, s), [u16(x) for x in inputs])).copy()


def assert_half(dt: int, got, want, what: str = "") -> None:
    got, want = u16(got), u16(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    gn, wn = isnan(dt, got), isnan(dt, want)
    if not np.array_equal(gn, wn):
        idx = np.nonzero(gn != wn)[0][:8]
        raise AssertionError(f"{what}: NaN class differs at {idx}: got "
                             f"{[hex(v) for v in got[idx]]} want {[hex(v) for v in want[idx]]}")
    diff = (got != want) & ~gn
    if diff.any():
        idx = np.nonzero(diff)[0][:8]
        raise AssertionError(f"{what}: {int(diff.sum())} lanes differ, e.g. {idx}: got "
                             f"{[hex(v) for v in got[idx]]} want {[hex(v) for v in want[idx]]}")


# ±0, ±smallest / ±largest subnormal, ±smallest normal, ±1, ±largest finite,
# ±inf, a quiet NaN, and tie makers: 1 + ulp, 0.5 and 1.5 (products that land
# half-way, also in the subnormal range), the power of two whose ulp is 2 (its
# sums with 1 are ties), ~1/3 and ~pi
SPECIALS = {
    FLOAT16: [0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x8400,
              0x3C00, 0xBC00, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00,
              0x3C01, 0xBC01, 0x3800, 0x3E00, 0xBE00, 0x6800, 0xE800, 0x6801,
              0x3555, 0x4248, 0x0401, 0x1400, 0x9400, 0x7800, 0xF800, 0x0200, 0x8200],
    BFLOAT16: [0x0000, 0x8000, 0x0001, 0x8001, 0x007F, 0x807F, 0x0080, 0x8080,
               0x3F80, 0xBF80, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x7FC0,
               0x3F81, 0xBF81, 0x3F00, 0x3FC0, 0xBFC0, 0x4380, 0xC380, 0x4381,
               0x3EAB, 0x4049, 0x0081, 0x2000, 0xA000, 0x7F00, 0xFF00, 0x0040, 0x8040],
}


@functools.lru_cache(maxsize=None)
def grid(dt: int):
    """(dst, src): every 16-bit pattern against every special value, both
    ways round."""
    sp = np.array(SPECIALS[dt], np.uint16)
    every = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    a = np.repeat(every, sp.size)
    b = np.tile(sp, every.size)
    d, s = np.concatenate([a, b]), np.concatenate([b, a])
    d.setflags(write=False)
    s.setflags(write=False)
    return d, s


@functools.lru_cache(maxsize=None)
def grid_want(dt: int, op: int) -> np.ndarray:
    d, s = grid(dt)
    w = step(dt, op, d, s)
    w.setflags(write=False)
    return w


def patterns(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 65536, n, dtype=np.uint32).astype(np.uint16)


def uniform(dt: int, n: int, seed: int, lo: float = -1.0, hi: float = 1.0) -> np.ndarray:
    return from_float(dt, np.random.default_rng(seed).uniform(lo, hi, n))


def min_inputs(dt: int, n: int, seed: int) -> np.ndarray:
    """Drawn from {0, -0, 1, NaN}."""
    pool = np.array([0x0000, 0x8000, ONE[dt], INF[dt] | 0x0200 if dt == FLOAT16 else 0x7FC0],
                    np.uint16)
    return pool[np.random.default_rng(seed).integers(0, 4, n)]
