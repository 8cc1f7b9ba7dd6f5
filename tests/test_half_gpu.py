"""FI_FLOAT16 / FI_BFLOAT16 reduction on the GPU: the combine kernels (vector
body, element and byte-misaligned paths), the fused tree, the tree-put
kernel, the collectives' schedules and the one-shot kernels across processes.

The reference is tests/_half_ref.py (numpy float16, float32 + the
round-to-nearest-even shift for bf16; no product code).  NaN lanes must be NaN
on both sides; every other lane is bit-exact.
"""
import os
import queue

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from libfabric_amd import atomic
from tests import _half_ref as R

pytestmark = pytest.mark.gpu

HALF = (R.FLOAT16, R.BFLOAT16)
GUARD = 64          # elements on either side of a device operand (128 bytes)
FILL = 0xA5


def _dev(x: np.ndarray, off: int = 0, odd: bool = False):
    """x on the device at element offset `off` from a 16-byte boundary (plus
    one byte when `odd`), with guard bytes around it: (whole buffer, view)."""
    x = R.u16(x)
    lead = (GUARD + off) * 2 + (1 if odd else 0)
    buf = torch.full((lead + x.nbytes + GUARD * 2 + 16,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[lead:lead + x.nbytes]
    view.copy_(torch.from_numpy(x.view(np.uint8).copy()))
    return buf, view


def _host(view: torch.Tensor) -> np.ndarray:
    return view.cpu().numpy().copy().view(np.uint16)


def _guards_intact(buf: torch.Tensor, view: torch.Tensor) -> bool:
    lead = view.storage_offset()        # (an empty view has no data pointer)
    b = buf.cpu().numpy()
    return bool((b[:lead] == FILL).all() and (b[lead + view.numel():] == FILL).all())


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("op", [R.SUM, R.PROD, R.MIN, R.MAX, R.LXOR, R.WRITE])
def test_write_special_value_grid(dt, op):
    d, s = R.grid(dt)
    db, dv = _dev(d)
    _, sv = _dev(s)
    atomic.write(op, dt, dv, sv)
    torch.cuda.synchronize()
    R.assert_half(dt, _host(dv), R.grid_want(dt, op), f"grid {R.NAMES[dt]} op={op}")
    assert np.array_equal(_host(sv), s)
    assert _guards_intact(db, dv)


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("op", [R.SUM, R.MIN])
def test_write_sizes_and_alignment(dt, op):
    big = (1 << 20) + 5
    d0, s0 = R.patterns(big, 3 + dt), R.patterns(big, 5 + op)
    want0 = R.step(dt, op, d0, s0)      # element-wise: a prefix's result is the prefix
    for n in (0, 1, 7, 1000, 4099, big):
        for doff, soff in ((0, 0), (1, 1), (3, 3), (7, 7), (1, 2), (0, 5)):
            db, dv = _dev(d0[:n], doff)
            sb, sv = _dev(s0[:n], soff)
            if n:
                assert dv.data_ptr() % 16 == 2 * doff and sv.data_ptr() % 16 == 2 * soff
            atomic.write(op, dt, dv, sv, n)
            torch.cuda.synchronize()
            what = f"{R.NAMES[dt]} op={op} n={n} offs=({doff},{soff})"
            R.assert_half(dt, _host(dv), want0[:n], what)
            assert _guards_intact(db, dv) and _guards_intact(sb, sv), what
            assert np.array_equal(_host(sv), s0[:n]), what
    n = 3001                            # odd byte addresses
    db, dv = _dev(d0[:n], 0, odd=True)
    sb, sv = _dev(s0[:n], 2, odd=True)
    assert dv.data_ptr() % 2 == 1 and sv.data_ptr() % 2 == 1
    atomic.write(op, dt, dv, sv, n)
    torch.cuda.synchronize()
    R.assert_half(dt, dv.cpu().numpy().copy(), want0[:n], "odd byte address")
    assert _guards_intact(db, dv) and _guards_intact(sb, sv)


SUBNORMAL = {
    # (op, dst, src, result): results in the subnormal range are produced, not flushed
    R.FLOAT16: [(R.SUM, 0x0001, 0x0001, 0x0002), (R.SUM, 0x03FF, 0x0001, 0x0400),
                (R.SUM, 0x8001, 0x0003, 0x0002), (R.PROD, 0x0400, 0x3800, 0x0200),
                (R.PROD, 0x0003, 0x3800, 0x0002), (R.PROD, 0x0001, 0x3800, 0x0000),
                (R.PROD, 0x1400, 0x1400, 0x0010), (R.MIN, 0x0002, 0x0001, 0x0001)],
    R.BFLOAT16: [(R.SUM, 0x0001, 0x0001, 0x0002), (R.SUM, 0x007F, 0x0001, 0x0080),
                 (R.SUM, 0x8001, 0x0003, 0x0002), (R.PROD, 0x0080, 0x3F00, 0x0040),
                 (R.PROD, 0x2000, 0x2000, 0x0080), (R.PROD, 0x1F80, 0x2000, 0x0040),
                 (R.PROD, 0x0003, 0x3F00, 0x0002), (R.MAX, 0x0001, 0x0002, 0x0002)],
}


@pytest.mark.parametrize("dt", HALF)
def test_subnormals_kept(dt):
    for op, d, s, r in SUBNORMAL[dt]:
        one = R.step(dt, op, np.array([d], np.uint16), np.array([s], np.uint16))
        assert int(one[0]) == r, (hex(d), hex(s), hex(int(one[0])), hex(r))   # the reference agrees
        for n, off in ((4096, 0), (3, 1)):       # the vector body, the element path
            _, dv = _dev(np.full(n, d, np.uint16), off)
            _, sv = _dev(np.full(n, s, np.uint16), off)
            atomic.write(op, dt, dv, sv, n)
            torch.cuda.synchronize()
            got = _host(dv)
            assert (got == r).all(), (R.NAMES[dt], op, hex(d), hex(s), hex(int(got[0])), hex(r), n)


def _tree_inputs(dt, op, nsrc, n, seed):
    gen = R.uniform if op == R.SUM else R.min_inputs
    return [gen(dt, n, seed + 31 * nsrc + k) for k in range(nsrc)]


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("op", [R.SUM, R.MIN])
def test_reduce_tree(dt, op):
    n = 10_003
    for nsrc in (1, 2, 3, 5, 8, 9, 16, 17, 31, 32):
        ins = _tree_inputs(dt, op, nsrc, n, 1000)
        want = R.tree(dt, op, ins)
        what = f"tree {R.NAMES[dt]} op={op} nsrc={nsrc}"
        devs = [_dev(x) for x in ins]
        ob, ov = _dev(np.zeros(n, np.uint16))
        atomic.reduce_tree(op, dt, ov, [v for _, v in devs], n)
        torch.cuda.synchronize()
        R.assert_half(dt, _host(ov), want, what)
        assert _guards_intact(ob, ov), what
        for (_, v), x in zip(devs, ins):
            assert np.array_equal(_host(v), x), what        # inputs untouched
        # in place, into the highest rank's buffer
        atomic.reduce_tree(op, dt, devs[-1][1], [v for _, v in devs], n)
        torch.cuda.synchronize()
        R.assert_half(dt, _host(devs[-1][1]), want, what + " in place")
        assert _guards_intact(*devs[-1]), what


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("nsrc,ndst", [(2, 1), (3, 2), (8, 7), (8, 8), (17, 2), (32, 32)])
def test_reduce_tree_put(dt, nsrc, ndst):
    n, off = 70_003, 3                  # a misaligned head of 5 elements
    for op in (R.SUM, R.MIN):
        ins = _tree_inputs(dt, op, nsrc, n, 2000)
        want = R.tree(dt, op, ins)
        srcs = [_dev(x, off) for x in ins]
        outs = [_dev(np.zeros(n, np.uint16), off) for _ in range(ndst)]
        atomic.reduce_tree_put(op, dt, [v for _, v in outs], [v for _, v in srcs], n)
        torch.cuda.synchronize()
        for j, (b, v) in enumerate(outs):
            what = f"tree_put {R.NAMES[dt]} op={op} {nsrc}->{ndst} out={j}"
            R.assert_half(dt, _host(v), want, what)
            assert _guards_intact(b, v), what
        for (b, v), x in zip(srcs, ins):
            assert np.array_equal(_host(v), x) and _guards_intact(b, v)


ALLREDUCE, REDUCE_SCATTER, REDUCE = 3, 5, 6


@pytest.mark.parametrize("n", [2, 3, 8])
@pytest.mark.parametrize("dt,op", [(R.BFLOAT16, R.SUM), (R.FLOAT16, R.PROD)])
def test_loopback_every_algorithm(n, dt, op):
    from libfabric_amd import coll
    for count in (1, 777, 100_003):
        lo, hi = (0.9, 1.1) if op == R.PROD else (-1.0, 1.0)
        sends = [R.uniform(dt, count, 7 * n + count + k, lo, hi) for k in range(n)]
        want = R.tree(dt, op, sends)
        sd = [_dev(x)[1] for x in sends]
        for algo in (0, 1, 3, 4):
            what = f"{R.NAMES[dt]} op={op} n={n} count={count} algo={algo}"
            rd = [_dev(np.zeros(count, np.uint16)) for _ in range(n)]
            coll.loopback(ALLREDUCE, algo, n, -1, dt, op, count, sd, [v for _, v in rd])
            torch.cuda.synchronize()
            for r, (b, v) in enumerate(rd):
                R.assert_half(dt, _host(v), want, f"allreduce {what} r={r}")
                assert _guards_intact(b, v), what
            blocks = [coll.block(count, n, r) for r in range(n)]
            rd = [_dev(np.zeros(ln, np.uint16)) for _, ln in blocks]
            coll.loopback(REDUCE_SCATTER, algo, n, -1, dt, op, count, sd, [v for _, v in rd])
            torch.cuda.synchronize()
            for r, (b, v) in enumerate(rd):
                o, ln = blocks[r]
                R.assert_half(dt, _host(v), want[o:o + ln], f"reduce_scatter {what} r={r}")
                assert _guards_intact(b, v), what
            root = n - 1
            rd = [_dev(np.zeros(count, np.uint16)) for _ in range(n)]
            coll.loopback(REDUCE, algo, n, root, dt, op, count, sd, [v for _, v in rd])
            torch.cuda.synchronize()
            R.assert_half(dt, _host(rd[root][1]), want, f"reduce {what}")
        for v, x in zip(sd, sends):
            assert np.array_equal(_host(v), x)


def test_tree_equals_chained_pairwise_writes():
    """nsrc = 8 bf16 SUM: the fused tree gives the bits of seven pairwise
    combines issued in its order (leaves, then higher OP lower per level)."""
    dt, op, n = R.BFLOAT16, R.SUM, 10_003
    ins = _tree_inputs(dt, op, 8, n, 3000)
    _, ov = _dev(np.zeros(n, np.uint16))
    atomic.reduce_tree(op, dt, ov, [_dev(x)[1] for x in ins], n)
    parts = [_dev(x)[1] for x in ins]
    calls = 0
    while len(parts) > 1:
        nxt = []
        for j in range(len(parts) // 2):
            atomic.write(op, dt, parts[2 * j + 1], parts[2 * j], n)   # higher OP= lower
            nxt.append(parts[2 * j + 1])
            calls += 1
        parts = nxt
    torch.cuda.synchronize()
    assert calls == 7
    assert np.array_equal(_host(parts[0]), _host(ov))
    R.assert_half(dt, _host(ov), R.tree(dt, op, ins), "tree")


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _oneshot_worker(rank, world, port, q, ll):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LFA_DEBUG="1",
                          LFA_OS_LL=ll)
        from test_coll_peer_gpu import _ready, _share_gpu
        _share_gpu(world)
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from gloo_xfer import GlooXfer
        from libfabric_amd import coll
        ep = coll.HostEndpoint(rank, world, GlooXfer(), device=0)
        ncase = 0
        try:
            ep.set_algo(coll.ALGO_P2P)
            for dt in HALF:
                sp = np.array(R.SPECIALS[dt], np.uint16)
                for op in (R.SUM, R.MIN, R.PROD):
                    n = 1531                    # 3062 bytes: under 4 KiB, ragged blocks
                    # edge values against each other, rotated per rank, then patterns
                    sends = [np.concatenate([np.roll(np.tile(sp, 8), 5 * k)[:256],
                                             R.patterns(n - 256, 40 + 3 * k + op)])
                             for k in range(world)]
                    want = R.tree(dt, op, sends)
                    what = f"{R.NAMES[dt]} op={op} world={world} ll={ll}"
                    x = torch.from_numpy(sends[rank].view(np.uint8).copy()).cuda()
                    r = torch.zeros_like(x)
                    _ready()
                    ep.wait(ep.allreduce(x, r, n, dt, op))
                    R.assert_half(dt, r.cpu().numpy(), want, "allreduce " + what)
                    off, ln = coll.block(n, world, rank)
                    rs = torch.zeros(max(ln, 1) * 2, dtype=torch.uint8, device="cuda")
                    _ready()
                    ep.wait(ep.reduce_scatter(x, rs, n, dt, op))
                    R.assert_half(dt, rs[:ln * 2].cpu().numpy(), want[off:off + ln],
                                  "reduce_scatter " + what)
                    root = ncase % world
                    rr = torch.zeros_like(x)
                    _ready()
                    ep.wait(ep.reduce(x, rr if rank == root else None, n, root, dt, op))
                    if rank == root:
                        R.assert_half(dt, rr.cpu().numpy(), want, "reduce " + what)
                    ncase += 1
            cnt = ep.counters()
            if world > 1:   # every one of them ran as the one-shot kernel
                assert cnt["oneshot"] == 3 * ncase and not cnt["timed_out"], cnt
        finally:
            ep.close()
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, f"ok {ncase}"))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("world,ll", [(1, "0"), (2, "0"), (2, "1"), (5, "0"), (5, "1")])
def test_oneshot_across_processes(world, ll):
    """LFA_ALGO_P2P's one-shot allreduce / reduce_scatter / reduce of both
    types across processes sharing the GPU (ll "1": the LL kernel for the
    allreduce and reduce_scatter parts); one process takes the copy path."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_oneshot_worker, args=(r, world, port, q, ll))
             for r in range(world)]
    for p in procs:
        p.start()
    results = {}
    try:
        for _ in range(world):
            try:
                r, msg = q.get(timeout=140)
            except queue.Empty:         # a rank hung: report the others
                break
            results[r] = msg
    finally:
        for p in procs:
            p.join(timeout=5)
            if p.is_alive():
                p.kill()
    bad = {r: results.get(r) for r in range(world) if not str(results.get(r)).startswith("ok")}
    assert not bad, "\n".join(f"rank {r}: {m}" for r, m in sorted(bad.items()))
