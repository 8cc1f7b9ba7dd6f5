"""The fetch and compare list (fi_ioc) forms on the GPU: one launch for a list
of segments must give, bit for bit, what one lfa_atomic_readwrite_async /
lfa_atomic_swap_async per segment gives, and what the oracle's fetch / compare
functions give: res is the old dst, dst is updated.

Every operand of a call has its own arena with 64 sentinel bytes between
segments (tests/_iov_fetch_layout.py); after every call every gap still holds
the sentinel.  NaN lanes must be NaN on both sides, every other lane is
bit-exact (tests/_cmp.py)."""
import ctypes

import numpy as np
import pytest
import torch

from libfabric_amd import _native, atomic
from tests import _iov_fetch_layout as F
from tests import _iov_layout as L
from tests import _sweep
from tests._cmp import assert_parity

pytestmark = pytest.mark.gpu

EINVAL, EOPNOTSUPP = -22, -95
FETCH, COMPARE = ("dst", "src", "res"), ("dst", "src", "cmp", "res")


@pytest.fixture(scope="module", autouse=True)
def _forms_present():
    assert hasattr(_native.lib(), "lfa_atomic_swapv_async"), "the list forms are missing"


def _dev(a: np.ndarray) -> torch.Tensor:
    t = torch.from_numpy(a.copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _views(t: torch.Tensor, segs):
    return [t[lo:lo + nb] for lo, nb in segs]


def _same(dt, got: np.ndarray, want: np.ndarray, segs, what):
    assert L.gaps_intact(got, segs), f"{what}: a gap lost its sentinel"
    for i, (lo, nb) in enumerate(segs):
        assert_parity(dt, got[lo:lo + nb].copy(), want[lo:lo + nb].copy(), f"{what} seg {i}")


def _oracle(op, dt, ar, names):
    """(new dst arena, res arena) from the oracle, segment by segment."""
    (dsegs, d0), (ssegs, s0), (rsegs, r0) = ar["dst"], ar["src"], ar["res"]
    d, r = d0.copy(), r0.copy()
    for i, ((dlo, nb), (slo, _), (rlo, _)) in enumerate(zip(dsegs, ssegs, rsegs)):
        if not nb:
            continue
        old, src = d0[dlo:dlo + nb], s0[slo:slo + nb]
        if "cmp" in names:
            clo = ar["cmp"][0][i][0]
            d[dlo:dlo + nb] = _sweep.reference_swap(op, dt, old, src, ar["cmp"][1][clo:clo + nb])
        else:
            d[dlo:dlo + nb] = _sweep.reference_readwrite(op, dt, old, src)
        r[rlo:rlo + nb] = old
    return d, r


def _run_both(op, dt, ar, names, what):
    """The list call and the loop of contiguous calls on copies of `ar`; every
    operand of both compared, and the list call against the oracle."""
    segs = {n: s for n, (s, _) in ar.items()}
    got = {n: _dev(a) for n, (_, a) in ar.items()}
    want = {n: _dev(a) for n, (_, a) in ar.items()}
    wv = {n: _views(want[n], segs[n]) for n in names}
    for i in range(len(segs["dst"])):
        if "cmp" in names:
            atomic.swap(op, dt, wv["dst"][i], wv["src"][i], wv["cmp"][i], wv["res"][i])
        else:
            atomic.readwrite(op, dt, wv["dst"][i], wv["src"][i], wv["res"][i])
    gv = [_views(got[n], segs[n]) for n in names]
    (atomic.swapv if "cmp" in names else atomic.readwritev)(op, dt, *gv)
    torch.cuda.synchronize()
    host = {n: got[n].cpu().numpy() for n in names}
    for n in names:
        _same(dt, host[n], want[n].cpu().numpy(), segs[n], f"{what} {n} vs loop")
    for n in names[1:-1]:
        assert np.array_equal(host[n], ar[n][1]), f"{what}: {n} was written"
    od, orr = _oracle(op, dt, ar, names)
    _same(dt, host["dst"], od, segs["dst"], f"{what} dst vs oracle")
    _same(dt, host["res"], orr, segs["res"], f"{what} res vs oracle")
    return host


@pytest.mark.parametrize("compare", [False, True], ids=["fetch", "compare"])
@pytest.mark.parametrize("nseg", [1, 2, 37])
@pytest.mark.parametrize("dt", F.DTS)
def test_list_form_equals_loop_and_oracle(dt, nseg, compare):
    esz, names = F.ESZ[dt], COMPARE if compare else FETCH
    ops = F.valid_ops(atomic, dt, compare)
    assert len(ops) >= (5 if compare else 9)
    for op in ops:
        counts, offs = F.layout(nseg, esz, shift=op if nseg > 2 else 0)
        ar = F.arenas(counts, offs, esz, names, 300 + 13 * op + nseg, dt)
        host = _run_both(op, dt, ar, names, f"op={op} dt={dt} nseg={nseg}")
        if op != F.ATOMIC_READ:
            assert not np.array_equal(host["dst"], ar["dst"][1]), (op, dt, nseg)


@pytest.mark.parametrize("compare", [False, True], ids=["fetch", "compare"])
def test_layouts_reach_every_path(compare):
    """From the layouts alone (the test above uses the same): over the six
    datatypes the vector, element and byte-wise paths each occur, and on the
    vector path a head, a tail and a segment of at least three tiles."""
    names, seen = COMPARE if compare else FETCH, {}
    for dt in F.DTS:
        esz = F.ESZ[dt]
        for op in F.valid_ops(atomic, dt, compare):
            counts, offs = F.layout(37, esz, shift=op)
            seen.setdefault(esz, []).extend(p for p in F.paths(counts, offs, esz, names) if p)
    assert set(seen) == {1, 2, 4, 8, 16}
    F.assert_paths(seen)
    assert F.big(4) * 4 > 3 * L.TILE


def test_one_operand_breaks_co_alignment():
    """Segments of 4097 floats: res alone 4 bytes off in one, cmp alone in the
    next, and everything co-aligned in a third.  The path is decided over all
    of a segment's operands: the first two are on the element path."""
    counts = [4097, 4097, 4097]
    offs = {n: [8, 8, 8] for n in F.NAMES}
    offs["res"][0] = 12
    offs["cmp"][1] = 4
    kinds = [p[0] for p in F.paths(counts, offs, 4, COMPARE)]
    assert kinds == ["element", "element", "vector"]
    ar = F.arenas(counts, offs, 4, COMPARE, 71, L.FLOAT)
    _run_both(F.CSWAP, L.FLOAT, ar, COMPARE, "cswap, res / cmp off dst's alignment")
    # the fetch form: res alone, src alone
    offs["src"][1] = 4
    assert [p[0] for p in F.paths(counts, offs, 4, FETCH)] == ["element", "element", "vector"]
    ar = F.arenas(counts, offs, 4, FETCH, 72, L.FLOAT)
    _run_both(L.SUM, L.FLOAT, ar, FETCH, "sum, res / src off dst's alignment")


@pytest.mark.parametrize("compare", [False, True], ids=["fetch", "compare"])
def test_mixed_sizes(compare):
    """One segment of 8 MiB + 3 elements among 100 of 1..17 elements, shuffled."""
    names = COMPARE if compare else FETCH
    rng = np.random.default_rng(5)
    counts = [int(c) for c in rng.integers(1, 18, 100)] + [(8 << 20) // 4 + 3]
    counts = [counts[i] for i in rng.permutation(len(counts))]
    o = [int(x) for x in rng.choice([0, 4, 8, 12], len(counts))]
    offs = {n: list(o) for n in F.NAMES}
    ar = F.arenas(counts, offs, 4, names, 41, L.FLOAT)
    _run_both(F.CSWAP if compare else L.SUM, L.FLOAT, ar, names, "mixed sizes")


@pytest.mark.parametrize("compare", [False, True], ids=["fetch", "compare"])
@pytest.mark.parametrize("two_tile", [False, True], ids=["direct", "search"])
def test_iov_max_segments(compare, two_tile):
    """LFA_IOV_MAX one-element segments: workgroup b owns segment b.  With one
    two-tile segment among them every workgroup searches the prefix table, 12
    steps deep."""
    names = COMPARE if compare else FETCH
    n = atomic.LFA_IOV_MAX
    counts = [1] * n
    if two_tile:
        counts[n // 3] = L.TILE // 4 + 8       # past its head still more than one tile
    offs = {name: [0, 4, 8, 12] * (n // 4) for name in F.NAMES}
    ar = F.arenas(counts, offs, 4, names, 51, L.INT32)
    tiles = [p[3] for p in F.paths(counts, offs, 4, names)]
    assert sum(tiles) == n + two_tile and max(tiles) == 1 + two_tile
    _run_both(F.CSWAP if compare else L.SUM, L.INT32, ar, names, f"{n} segments")


def _lists(tensors, segs, names, esz):
    out = []
    for n in names:
        a = (_native.lfa_ioc * len(segs[n]))()
        for i, (lo, nb) in enumerate(segs[n]):
            a[i].addr, a[i].count = tensors[n].data_ptr() + lo, nb // esz
        out.append(a)
    return out


@pytest.mark.parametrize("compare", [False, True], ids=["fetch", "compare"])
def test_host_arrays_may_be_reused_on_return(compare):
    """Two calls back to back on one non-default stream (a ring-slot table, an
    in-argument table), the caller's arrays overwritten as soon as each
    returns, one synchronisation at the end."""
    lib = _native.lib()
    names = COMPARE if compare else FETCH
    op = F.CSWAP if compare else L.SUM
    stream = torch.cuda.Stream()
    jobs = []
    for nseg, seed in ((37, 61), (3, 63)):
        counts, offs = F.layout(nseg, 4, shift=2)
        ar = F.arenas(counts, offs, 4, names, seed, L.FLOAT)
        segs = {n: s for n, (s, _) in ar.items()}
        got = {n: _dev(a) for n, (_, a) in ar.items()}
        jobs.append((ar, segs, got))
    torch.cuda.synchronize()
    for ar, segs, got in jobs:
        lists = _lists(got, segs, names, 4)
        fn = lib.lfa_atomic_swapv_async if compare else lib.lfa_atomic_readwritev_async
        assert fn(op, L.FLOAT, *lists, len(segs["dst"]), stream.cuda_stream) == 0
        for a in lists:
            ctypes.memset(a, 0xEE, ctypes.sizeof(a))
    stream.synchronize()
    for ar, segs, got in jobs:
        od, orr = _oracle(op, L.FLOAT, ar, names)
        _same(L.FLOAT, got["dst"].cpu().numpy(), od, segs["dst"], "dst")
        _same(L.FLOAT, got["res"].cpu().numpy(), orr, segs["res"], "res")


@pytest.mark.parametrize("compare", [False, True], ids=["fetch", "compare"])
def test_more_ring_calls_in_flight_than_slots(compare):
    """20 calls whose tables go through the ring (8 slots per device), enqueued
    behind about 2 ms of other work on the stream so that they are all in
    flight at once.  Every call has its own arenas, so a table that reached the
    wrong launch shows in two of them."""
    names = COMPARE if compare else FETCH
    op = F.CSWAP if compare else L.SUM
    counts, offs = F.layout(37, 4, shift=5)
    jobs = []
    for c in range(20):
        ar = F.arenas(counts, offs, 4, names, 100 + 5 * c, L.FLOAT)
        segs = {n: s for n, (s, _) in ar.items()}
        jobs.append((ar, segs, {n: _dev(a) for n, (_, a) in ar.items()}))
    ahead = torch.zeros(256 << 20, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for _ in range(16):
        ahead.add_(1)
    for ar, segs, got in jobs:
        gv = [_views(got[n], segs[n]) for n in names]
        (atomic.swapv if compare else atomic.readwritev)(op, L.FLOAT, *gv)
    torch.cuda.synchronize()
    for c, (ar, segs, got) in enumerate(jobs):
        od, orr = _oracle(op, L.FLOAT, ar, names)
        _same(L.FLOAT, got["dst"].cpu().numpy(), od, segs["dst"], f"call {c} dst")
        _same(L.FLOAT, got["res"].cpu().numpy(), orr, segs["res"], f"call {c} res")


@pytest.mark.parametrize("nseg", [1, 2, 37])
def test_atomic_read_without_src(nseg):
    """ATOMIC_READ with src = NULL: dst is unchanged and res equals dst."""
    counts, offs = F.layout(nseg, 4, shift=1)
    names = ("dst", "res")
    ar = F.arenas(counts, offs, 4, names, 81, L.FLOAT)
    segs = {n: s for n, (s, _) in ar.items()}
    got = {n: _dev(a) for n, (_, a) in ar.items()}
    atomic.readwritev(F.ATOMIC_READ, L.FLOAT, _views(got["dst"], segs["dst"]), None,
                      _views(got["res"], segs["res"]))
    torch.cuda.synchronize()
    d, r = got["dst"].cpu().numpy(), got["res"].cpu().numpy()
    assert np.array_equal(d, ar["dst"][1])
    assert L.gaps_intact(r, segs["res"])
    for (dlo, nb), (rlo, _) in zip(segs["dst"], segs["res"]):
        assert np.array_equal(r[rlo:rlo + nb], d[dlo:dlo + nb])
    assert not np.array_equal(r, ar["res"][1])


def test_errors_launch_nothing():
    counts, o = [16, 16, 16], [0, 4, 8]
    offs = {n: list(o) for n in F.NAMES}
    ar = F.arenas(counts, offs, 4, COMPARE, 91, L.FLOAT)
    segs = ar["dst"][0]
    t = {n: _dev(a) for n, (_, a) in ar.items()}
    v = {n: _views(t[n], segs) for n in COMPARE}

    def refused(rc, fn, *args):
        with pytest.raises(atomic.LfaError) as e:
            fn(*args)
        assert e.value.rc == rc
        torch.cuda.synchronize()
        for n in COMPARE:
            assert np.array_equal(t[n].cpu().numpy(), ar[n][1]), n
    lo = segs[0][0]
    d, s, c, r = v["dst"], v["src"], v["cmp"], v["res"]
    over = [d[0], t["dst"][lo + 60:lo + 124], d[2]]                 # dst[1] overlaps dst[0]
    res_in_dst = [r[0], t["dst"][segs[1][0] + 32:segs[1][0] + 96], r[2]]    # res[1] overlaps dst[1]
    res_in_res = [r[0], t["res"][lo + 60:lo + 124], r[2]]           # res[1] overlaps res[0]
    for fn, mid in ((atomic.readwritev, ()), (atomic.swapv, (c,))):
        op = F.CSWAP if mid else L.SUM
        refused(EINVAL, fn, op, L.FLOAT, over, s, *mid, r)
        refused(EINVAL, fn, op, L.FLOAT, d, s, *mid, res_in_dst)
        refused(EINVAL, fn, op, L.FLOAT, d, s, *mid, res_in_res)
        refused(EINVAL, fn, op, L.FLOAT, d, [s[0], s[1][:60], s[2]], *mid, r)
        refused(EINVAL, fn, op, L.FLOAT, d, s, *mid, [r[0], r[1][:60], r[2]])
        refused(EOPNOTSUPP, fn, L.BXOR, L.FLOAT, d, s, *mid, r)
        refused(EOPNOTSUPP, fn, op, 17, d, s, *mid, r)              # no 16-bit float form
        one = t["dst"][lo:lo + 4]
        many = [one] * (atomic.LFA_IOV_MAX + 1)
        refused(EINVAL, fn, op, L.FLOAT, many, many, *((many,) if mid else ()), many)
    refused(EINVAL, atomic.swapv, F.CSWAP, L.FLOAT, d, s, [c[0], c[1][:60], c[2]], r)
    refused(EINVAL, atomic.readwritev, L.SUM, L.FLOAT, d, None, r)  # only ATOMIC_READ has no src
    with pytest.raises(ValueError):
        atomic.readwritev(L.SUM, L.FLOAT, [torch.from_numpy(ar["dst"][1])], [s[0]], [r[0]])
