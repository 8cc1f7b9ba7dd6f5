"""The list (fi_ioc) forms on the GPU: one launch for a list of segments must
give, bit for bit, what one launch per segment gives.

Every call's segments are carved from one arena with 64 sentinel bytes
between them (tests/_iov_layout.py); after every call every gap still holds
the sentinel.  NaN lanes must be NaN on both sides, every other lane is
bit-exact (tests/_cmp.py, tests/_half_ref.py)."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from libfabric_amd import _native, atomic
from tests import _half_ref as R
from tests import _iov_layout as L
from tests._cmp import assert_parity

pytestmark = pytest.mark.gpu

EINVAL, EOPNOTSUPP = -22, -95


def _dev(a: np.ndarray) -> torch.Tensor:
    t = torch.from_numpy(a.copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _views(t: torch.Tensor, segs):
    return [t[lo:lo + nb] for lo, nb in segs]


def _same(dt, got: np.ndarray, want: np.ndarray, segs, what):
    """Segment by segment: NaN-aware for the float types, else byte-exact."""
    assert L.gaps_intact(got, segs), f"{what}: a gap lost its sentinel"
    for i, (lo, nb) in enumerate(segs):
        g, w = got[lo:lo + nb].copy(), want[lo:lo + nb].copy()
        if dt == L.BFLOAT16:
            R.assert_half(dt, g.view(np.uint16), w.view(np.uint16), f"{what} seg {i}")
        else:
            assert_parity(dt, g, w, f"{what} seg {i}")


DTS = (L.INT8, L.BFLOAT16, L.FLOAT, L.DOUBLE, L.INT128, L.FLOAT_COMPLEX)
OPS = (L.SUM, L.MIN, L.PROD, L.LXOR, L.BXOR)


def _pairs(dt):
    for op in OPS:
        if op == L.BXOR and dt not in L.INTEGERS:
            continue
        if atomic.reduce_valid(dt, op) == 0:
            yield op


@pytest.mark.parametrize("nseg", [1, 2, 37])
@pytest.mark.parametrize("dt", DTS)
def test_writev_equals_loop(dt, nseg):
    esz = L.ESZ[dt]
    for op in _pairs(dt):
        # nseg 1 and 2: the 4097-element segment first, 2 bytes past a boundary
        counts, offsets, (segs, size) = L.standard(nseg, esz, shift=op if nseg > 2 else 7)
        # every third source starts where the next segment's dst does: aligned
        # to the element but not co-aligned with dst (the element loop), or
        # not aligned at all (byte-wise)
        soffs = [offsets[(i + 1) % nseg] if i % 3 == 2 else o for i, o in enumerate(offsets)]
        ssegs, ssize = L.plan(counts, soffs, esz)
        if nseg == 37:
            kinds = {p[0] for p in (L.path(esz, c, o, [so])
                                    for c, o, so in zip(counts, offsets, soffs)) if p}
            # a 1-byte element is never misaligned; 16-byte elements that are
            # aligned are co-aligned
            assert kinds == {"vector", "element", "bytes"} - {"bytes" if esz == 1 else "",
                                                              "element" if esz == 16 else ""}
        d0, s0 = L.fill(size, segs, 10 + op, dt), L.fill(ssize, ssegs, 20 + op, dt)
        got, want, src = _dev(d0), _dev(d0), _dev(s0)
        for d, s in zip(_views(want, segs), _views(src, ssegs)):
            atomic.write(op, dt, d, s)
        atomic.writev(op, dt, _views(got, segs), _views(src, ssegs))
        torch.cuda.synchronize()
        what = f"op={op} dt={dt} nseg={nseg}"
        _same(dt, got.cpu().numpy(), want.cpu().numpy(), segs, what)
        assert np.array_equal(src.cpu().numpy(), s0), what
        if sum(counts):
            assert not np.array_equal(got.cpu().numpy(), d0), what


@pytest.mark.parametrize("opname,dtname", [("SUM", "FLOAT"), ("MIN", "INT64")])
def test_writev_vs_oracle(opname, dtname):
    op, dt = oracle.OPS[opname], oracle.DT_CODE[dtname]
    esz, nd = oracle.datatype_size(dt), oracle.DT_NP[dt]
    _, _, (segs, size) = L.standard(37, esz, shift=1)
    d0, s0 = L.fill(size, segs, 31, dt), L.fill(size, segs, 32, dt)
    want = d0.copy()
    for lo, nb in segs:
        d, s = want[lo:lo + nb].copy().view(nd), s0[lo:lo + nb].copy().view(nd)
        oracle.write(op, dt, d, s)
        want[lo:lo + nb] = d.view(np.uint8)
    got, src = _dev(d0), _dev(s0)
    atomic.writev(op, dt, _views(got, segs), _views(src, segs))
    torch.cuda.synchronize()
    _same(dt, got.cpu().numpy(), want, segs, f"{opname} {dtname} vs oracle")


def test_mixed_sizes():
    """One segment of 8 MiB + 3 elements among 100 of 1..17 elements, shuffled:
    the tile table, the search and each segment's head and tail."""
    rng = np.random.default_rng(5)
    counts = [int(c) for c in rng.integers(1, 18, 100)] + [(8 << 20) // 4 + 3]
    order = rng.permutation(len(counts))
    counts = [counts[i] for i in order]
    offsets = [int(o) for o in rng.choice([0, 4, 8, 12], len(counts))]
    segs, size = L.plan(counts, offsets, 4)
    d0, s0 = L.fill(size, segs, 41, L.FLOAT), L.fill(size, segs, 42, L.FLOAT)
    got, want, src = _dev(d0), _dev(d0), _dev(s0)
    for d, s in zip(_views(want, segs), _views(src, segs)):
        atomic.write(L.SUM, L.FLOAT, d, s)
    atomic.writev(L.SUM, L.FLOAT, _views(got, segs), _views(src, segs))
    torch.cuda.synchronize()
    _same(L.FLOAT, got.cpu().numpy(), want.cpu().numpy(), segs, "mixed sizes")
    # the same list with the sources a further 4 bytes on: the big segment on
    # the element loop (dst and src no longer co-aligned)
    segs2, size2 = L.plan(counts, [(o + 4) % 16 for o in offsets], 4)
    s1 = L.fill(size2, segs2, 43, L.FLOAT)
    got, want, src = _dev(d0), _dev(d0), _dev(s1)
    for d, s in zip(_views(want, segs), _views(src, segs2)):
        atomic.write(L.SUM, L.FLOAT, d, s)
    atomic.writev(L.SUM, L.FLOAT, _views(got, segs), _views(src, segs2))
    torch.cuda.synchronize()
    _same(L.FLOAT, got.cpu().numpy(), want.cpu().numpy(), segs, "mixed sizes, not co-aligned")


def test_iov_max_segments():
    """LFA_IOV_MAX segments of 16 floats: the table's ring path to the device."""
    n = atomic.LFA_IOV_MAX
    segs, size = L.plan([16] * n, [0, 4] * (n // 2), 4)
    d0, s0 = L.fill(size, segs, 51, L.FLOAT), L.fill(size, segs, 52, L.FLOAT)
    want = d0.copy()
    for lo, nb in segs:
        want[lo:lo + nb] = (d0[lo:lo + nb].copy().view(np.float32) +
                            s0[lo:lo + nb].copy().view(np.float32)).view(np.uint8)
    got, src = _dev(d0), _dev(s0)
    for _ in range(2):      # twice: the second call reuses nothing of the first
        got.copy_(torch.from_numpy(d0))
        atomic.writev(L.SUM, L.FLOAT, _views(got, segs), _views(src, segs))
    torch.cuda.synchronize()
    g = got.cpu().numpy()
    assert L.gaps_intact(g, segs)
    idx = np.concatenate([np.arange(lo, lo + nb) for lo, nb in segs])
    assert_parity(L.FLOAT, g[idx], want[idx], "LFA_IOV_MAX segments")


def test_host_arrays_may_be_reused_on_return():
    """Two calls back to back on one non-default stream, the caller's arrays
    overwritten as soon as each returns, one synchronisation at the end."""
    lib = _native.lib()
    stream = torch.cuda.Stream()
    results = []
    for nseg, seed in ((37, 61), (3, 63)):      # a ring-slot table, an in-argument table
        _, _, (segs, size) = L.standard(nseg, 4, shift=2)
        d0, s0 = L.fill(size, segs, seed, L.FLOAT), L.fill(size, segs, seed + 1, L.FLOAT)
        got, want, src = _dev(d0), _dev(d0), _dev(s0)
        for d, s in zip(_views(want, segs), _views(src, segs)):
            atomic.write(L.SUM, L.FLOAT, d, s)
        results.append((segs, got, want, src))
    torch.cuda.synchronize()
    for segs, got, want, src in results:
        da = (_native.lfa_ioc * len(segs))()
        sa = (_native.lfa_ioc * len(segs))()
        for i, (lo, nb) in enumerate(segs):
            da[i].addr, da[i].count = got.data_ptr() + lo, nb // 4
            sa[i].addr, sa[i].count = src.data_ptr() + lo, nb // 4
        rc = lib.lfa_atomic_writev_async(L.SUM, L.FLOAT, da, sa, len(segs), stream.cuda_stream)
        assert rc == 0
        ctypes.memset(da, 0xEE, ctypes.sizeof(da))
        ctypes.memset(sa, 0xEE, ctypes.sizeof(sa))
    stream.synchronize()
    for segs, got, want, src in results:
        _same(L.FLOAT, got.cpu().numpy(), want.cpu().numpy(), segs, f"nseg={len(segs)}")


def test_more_ring_calls_in_flight_than_slots():
    """20 calls whose tables go through the ring (8 slots per device), enqueued
    behind about 2 ms of other work on the stream so that they are all in
    flight at once: a call that finds the oldest slot busy waits for it, and no
    table is overwritten before its kernel has read it.  Every call has its
    own arena, so a table that reached the wrong launch shows in two arenas."""
    ncall = 20
    _, _, (segs, size) = L.standard(37, 4, shift=5)
    jobs = []
    for c in range(ncall):
        d0, s0 = L.fill(size, segs, 100 + 2 * c, L.FLOAT), L.fill(size, segs, 101 + 2 * c, L.FLOAT)
        got, want, src = _dev(d0), _dev(d0), _dev(s0)
        for d, s in zip(_views(want, segs), _views(src, segs)):
            atomic.write(L.SUM, L.FLOAT, d, s)
        jobs.append((got, want, src))
    ahead = torch.zeros(256 << 20, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for _ in range(16):
        ahead.add_(1)
    for got, _, src in jobs:
        atomic.writev(L.SUM, L.FLOAT, _views(got, segs), _views(src, segs))
    torch.cuda.synchronize()
    for c, (got, want, _) in enumerate(jobs):
        _same(L.FLOAT, got.cpu().numpy(), want.cpu().numpy(), segs, f"call {c}")


TREE = ((L.SUM, L.FLOAT), (L.SUM, L.BFLOAT16), (L.PROD, L.DOUBLE), (L.BXOR, L.INT32))


# fan-ins of 1 (a copy), 2, 3 (odd: an unpaired leaf) and 8 (a node's GPUs)
# for all four pairs; 15 and 17 are either side of the threshold from which a
# call enqueues one tree launch per segment
@pytest.mark.parametrize("op,dt,nsrc",
                         [(op, dt, n) for op, dt in TREE for n in (1, 2, 3, 8)] +
                         [(L.SUM, L.FLOAT, 15), (L.SUM, L.FLOAT, 17)])
def test_treev_equals_loop(op, dt, nsrc):
    segs, size, in_k, paths = L.tree_layout(L.ESZ[dt], nsrc)
    if nsrc > 1:        # one input is a byte copy through the binary kernel
        L.assert_tree_paths(L.ESZ[dt], paths)
    d0 = L.fill(size, segs, 70 + nsrc, dt)
    seg_k = [sk for sk, _ in in_k]
    s0 = [L.fill(size_k, sk, 80 + 7 * nsrc + k, dt) for k, (sk, size_k) in enumerate(in_k)]
    got, want = _dev(d0), _dev(d0)
    src = [_dev(a) for a in s0]

    def rows(dst):
        dv = _views(dst, segs)
        out = []
        for i in range(len(segs)):
            row = [_views(src[k], seg_k[k])[i] for k in range(nsrc)]
            if i % 2 == 0:
                row[0] = dv[i]          # dst is its own first input
            out.append(row)
        return dv, out
    dv, rw = rows(want)
    for d, row in zip(dv, rw):
        atomic.reduce_tree(op, dt, d, row)
    dv, rw = rows(got)
    atomic.reduce_treev(op, dt, dv, rw)
    torch.cuda.synchronize()
    what = f"treev op={op} dt={dt} nsrc={nsrc}"
    _same(dt, got.cpu().numpy(), want.cpu().numpy(), segs, what)
    for k in range(nsrc):
        assert np.array_equal(src[k].cpu().numpy(), s0[k]), what
    if nsrc > 1:
        assert not np.array_equal(got.cpu().numpy(), d0), what


def test_errors_launch_nothing():
    segs, size = L.plan([16, 16, 16], [0, 4, 8], 4)
    d0, s0 = L.fill(size, segs, 91, L.FLOAT), L.fill(size, segs, 92, L.FLOAT)
    arena, src = _dev(d0), _dev(s0)
    dv, sv = _views(arena, segs), _views(src, segs)

    def refused(rc, fn, *args):
        with pytest.raises(atomic.LfaError) as e:
            fn(*args)
        assert e.value.rc == rc
        torch.cuda.synchronize()
        assert np.array_equal(arena.cpu().numpy(), d0) and np.array_equal(src.cpu().numpy(), s0)
    lo = segs[0][0]
    refused(EINVAL, atomic.writev, L.SUM, L.FLOAT, [dv[0], arena[lo + 60:lo + 124], dv[2]], sv)
    refused(EINVAL, atomic.writev, L.SUM, L.FLOAT, dv, [sv[0], sv[1][:60], sv[2]])
    refused(EOPNOTSUPP, atomic.writev, L.BXOR, L.FLOAT, dv, sv)
    one = arena[lo:lo + 4]
    many = [one] * (atomic.LFA_IOV_MAX + 1)
    refused(EINVAL, atomic.writev, L.SUM, L.FLOAT, many, many)
    refused(EINVAL, atomic.reduce_treev, L.SUM, L.FLOAT, [dv[0], arena[lo + 60:lo + 124]],
            [[sv[0], sv[1]], [sv[1], sv[2]]])
    refused(EOPNOTSUPP, atomic.reduce_treev, L.BXOR, L.FLOAT, dv[:2], [[sv[0], sv[1]]] * 2)
    with pytest.raises(ValueError):
        atomic.writev(L.SUM, L.FLOAT, [torch.from_numpy(d0)], [torch.from_numpy(s0)])  # host memory
