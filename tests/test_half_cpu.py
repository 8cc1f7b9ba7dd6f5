"""FI_FLOAT16 / FI_BFLOAT16 reduction, the parts that need no GPU: the two
predicate functions, the host combine (lfa_host_write / lfa_host_reduce_tree)
and the host-domain collectives.

The reference is tests/_half_ref.py: numpy float16, float32 + the
round-to-nearest-even shift for bf16, torch CPU as a second opinion.  NaN
lanes must be NaN on both sides; every other lane is bit-exact.
"""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import oracle
from libfabric_amd import atomic
from libfabric_amd.enums import DT, datatype_of_torch, torch_dtype_of
from tests import _half_ref as R

HALF = (R.FLOAT16, R.BFLOAT16)


def test_reference_second_opinions():
    """The two oracles agree with each other (SUM / PROD on random pattern
    pairs), and the tree restatement equals oracle.allreduce on float32 SUM
    for every input count the tests use."""
    for dt in HALF:
        d, s = R.patterns(1_000_000, 11 + dt), R.patterns(1_000_000, 23 + dt)
        for op in (R.SUM, R.PROD):
            R.assert_half(dt, R.step_torch(dt, op, d, s), R.step(dt, op, d, s),
                          f"torch vs numpy {R.NAMES[dt]} op={op}")
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 5, 8, 9, 16, 17, 31, 32):
        ins = [rng.uniform(-1, 1, 513).astype(np.float32) for _ in range(n)]
        want = oracle.allreduce(R.SUM, int(DT.FLOAT), ins)[0]
        got = R.tree_with(lambda a, b: a + b, ins)
        assert got.tobytes() == want.tobytes(), n


def test_reduce_valid_and_size():
    L = atomic.lib()
    for dt in range(16):
        assert atomic.reduce_datatype_size(dt) == atomic.datatype_size(dt), dt
        for op in range(20):
            assert atomic.reduce_valid(dt, op) == atomic.atomic_valid(dt, op, 0), (dt, op)
    for dt in HALF:
        assert atomic.reduce_datatype_size(dt) == 2
        for op in range(20):
            assert atomic.reduce_valid(dt, op) == (0 if op in R.OPS else -95), (dt, op)
        # the reference-shaped pair keeps its 16 columns
        assert atomic.datatype_size(dt) == 0
        for op in range(20):
            assert atomic.atomic_valid(dt, op, 0) == -95
    for dt in (18, 19, 20, 1000):
        ctypes.set_errno(0)
        assert L.lfa_reduce_datatype_size(dt) == 0
        assert atomic.reduce_valid(dt, R.SUM) == -95
    assert int(DT.FLOAT16) == 16 and int(DT.BFLOAT16) == 17
    import torch
    assert datatype_of_torch(torch.float16) == DT.FLOAT16
    assert datatype_of_torch(torch.bfloat16) == DT.BFLOAT16
    assert torch_dtype_of(DT.FLOAT16) == torch.float16
    assert torch_dtype_of(DT.BFLOAT16) == torch.bfloat16
    # no fetch / compare form, no bitwise op
    a = np.zeros(4, np.uint16)
    for op in (R.BOR, R.BAND, R.BXOR, R.READ):
        with pytest.raises(atomic.LfaError) as e:
            atomic.host_write(op, R.BFLOAT16, a, a)
        assert e.value.rc == -95
    assert L.lfa_host_readwrite(R.SUM, R.FLOAT16, None, None, None, 0) == -95


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("op", R.OPS)
def test_host_write(dt, op):
    d, s = R.grid(dt)
    got = d.copy()
    atomic.host_write(op, dt, got, s)
    R.assert_half(dt, got, R.grid_want(dt, op), f"grid {R.NAMES[dt]} op={op}")
    d, s = R.patterns(1_000_000, 100 + op), R.patterns(1_000_000, 200 + op + dt)
    got = d.copy()
    atomic.host_write(op, dt, got, s)
    R.assert_half(dt, got, R.step(dt, op, d, s), f"random {R.NAMES[dt]} op={op}")
    # odd addresses: operands not aligned to the element
    n = 3001
    d, s = R.patterns(n, 7 + op), R.patterns(n, 9 + op + dt)
    db, sb = np.zeros(2 * n + 3, np.uint8), np.zeros(2 * n + 5, np.uint8)
    db[1:1 + 2 * n] = d.view(np.uint8)
    sb[3:3 + 2 * n] = s.view(np.uint8)
    assert db[1:].ctypes.data % 2 == 1 and sb[3:].ctypes.data % 2 == 1
    atomic.host_write(op, dt, db[1:1 + 2 * n], sb[3:3 + 2 * n], n)
    R.assert_half(dt, db[1:1 + 2 * n].copy(), R.step(dt, op, d, s), "odd address")
    assert db[0] == 0 and db[-2:].tolist() == [0, 0]


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("op", [R.SUM, R.MIN])
@pytest.mark.parametrize("nsrc", [1, 2, 3, 5, 8, 17, 32])
def test_host_reduce_tree(dt, op, nsrc):
    n = 4099
    gen = R.uniform if op == R.SUM else R.min_inputs
    ins = [gen(dt, n, 31 * nsrc + k) for k in range(nsrc)]
    want = R.tree(dt, op, ins)
    if op == R.SUM and nsrc >= 8:
        # rounding after every step is visible: one rounding at the end differs
        once = R.narrow(dt, np.sum([R.widen(dt, x).astype(np.float64) for x in ins],
                                   axis=0).astype(np.float32))
        assert not np.array_equal(once, want)
    out = np.zeros(n, np.uint16)
    atomic.host_reduce_tree(op, dt, out, [x.copy() for x in ins])
    R.assert_half(dt, out, want, f"host tree {R.NAMES[dt]} op={op} nsrc={nsrc}")
    # in place, into the highest rank's buffer
    bufs = [x.copy() for x in ins]
    atomic.host_reduce_tree(op, dt, bufs[-1], bufs)
    R.assert_half(dt, bufs[-1], want, "in place")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _host_worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from gloo_xfer import GlooXfer
        from libfabric_amd import coll
        dt, op, count = R.BFLOAT16, R.SUM, 777
        sends = [R.uniform(dt, count, 50 + k) for k in range(world)]
        want = R.tree(dt, op, sends)
        ep = coll.HostEndpoint(rank, world, GlooXfer())
        try:
            for algo in (coll.ALGO_TREE, coll.ALGO_RD, coll.ALGO_TREE_COLL, coll.ALGO_P2P):
                ep.set_algo(algo)
                res = np.zeros(count, np.uint16)
                ep.wait(ep.allreduce(sends[rank].copy(), res, count, dt, op))
                R.assert_half(dt, res, want, f"allreduce algo={algo}")
                off, ln = coll.block(count, world, rank)
                res = np.zeros(max(ln, 1), np.uint16)
                ep.wait(ep.reduce_scatter(sends[rank].copy(), res, count, dt, op))
                R.assert_half(dt, res[:ln], want[off:off + ln], f"reduce_scatter algo={algo}")
                for root in range(world):
                    res = np.zeros(count, np.uint16)
                    ep.wait(ep.reduce(sends[rank].copy(), res, count, root, dt, op))
                    if rank == root:
                        R.assert_half(dt, res, want, f"reduce root={root} algo={algo}")
            # the non-reducing collectives carry the type as bytes
            x = R.patterns(10, 300 + rank)
            res = np.zeros(10 * world, np.uint16)
            ep.wait(ep.allgather(x, res, 10, R.FLOAT16))
            assert np.array_equal(res, np.concatenate([R.patterns(10, 300 + k)
                                                       for k in range(world)]))
            b = R.patterns(7, 400) if rank == world - 1 else np.zeros(7, np.uint16)
            ep.wait(ep.broadcast(b, 7, world - 1, dt))
            assert np.array_equal(b, R.patterns(7, 400))
            ep.wait(ep.barrier())
        finally:
            ep.close()
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("world", [2, 3])
def test_host_domain_collectives(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_host_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = {}
    try:
        for _ in range(world):
            r, msg = q.get(timeout=120)
            results[r] = msg
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    for r in range(world):
        assert results.get(r) == "ok", results.get(r)


def test_query_collective():
    from libfabric_amd import coll
    for dt in HALF:
        a = coll.CollectiveAttr(op=R.SUM, datatype=dt, mode=0)
        assert coll.lib().lfa_query_collective(None, int(coll.COLL.ALLREDUCE),
                                               ctypes.byref(a), 0) == 0
        assert a.datatype_attr.size == 2 and a.datatype_attr.count == (64 << 30) // 2
        a = coll.CollectiveAttr(op=R.BOR, datatype=dt, mode=0)
        assert coll.lib().lfa_query_collective(None, int(coll.COLL.ALLREDUCE),
                                               ctypes.byref(a), 0) == -95
        # a fetch / compare query of the 16-bit floats stays unsupported
        a = coll.CollectiveAttr(op=R.SUM, datatype=dt, mode=0)
        assert coll.lib().lfa_query_collective(None, int(coll.COLL.ALLREDUCE),
                                               ctypes.byref(a), 1 << 58) == -95
    a = coll.CollectiveAttr(op=R.SUM, datatype=int(DT.FLOAT), mode=0)
    assert coll.lib().lfa_query_collective(None, int(coll.COLL.ALLREDUCE),
                                           ctypes.byref(a), 0) == 0
    assert a.datatype_attr.size == 4
