"""Oracle sweep of every one-shot kernel instantiation, in one process.

launch_oneshot (lfa_k_launch.hpp) chooses among oneshot_reduce<OP, T, NLEAF>,
NLEAF 1, 2, 4, 8, and oneshot_ll<OP, T, NLEAF>, NLEAF 2, 4, 8
(lfa_k_oneshot.hpp): 931 instantiations over the 133 reducing pairs, the
kernels every small collective runs on.  tests/test_coll_peer_gpu.py runs
them across processes, with three operands in rotation (from 4 ranks on every
input is there twice, so MIN, MAX, BAND, BOR, LAND and LOR cannot see a leaf
dropped or read twice), in one workgroup, and sees only the final result.

Rank r's kernel waits only on its own workspace.  With the flags posted
beforehand no kernel ever waits, so here every rank's kernel runs one at a
time on one stream of this process (tests/_sweep.py os_run): pass 1 pushes and
posts, and what it wrote into every member's workspace is compared with the
inputs byte for byte, everything else in the workspaces still holding what was
there before (which areas changed also says which kernel ran); pass 2, same
epoch, reduces what pass 1 left, and every result is the oracle's under
assert_parity / assert_half, the sentinels around every send and result intact,
the inputs unchanged, no wait timed out.  The inputs are S.inputs (every input
visible in the result at 8 ranks, tests/test_sweep_cpu.py), the kernel is
chosen per call through lfa__oneshot_as, and no environment variable is set.

What this does not prove: visibility across processes, uncached workspaces,
ordering over xGMI.  tests/test_coll_peer_gpu.py stays the proof of those.

Each test counts its cases against a literal, so a skipped pair fails.
"""
import ctypes

import numpy as np
import pytest
import torch

from libfabric_amd import coll
from libfabric_amd.atomic import LFA_EINVAL, LFA_EOPNOTSUPP
from tests import _sweep as S

pytestmark = pytest.mark.gpu

OPS = range(10)
# 15 cases per pair (9 flagged, 6 LL) and 46 per op on one datatype each
# (folding 3, epochs 28, size edges 11, completion word 4)
N_CASES = 133 * 15 + 10 * 46


def _i32(x: int) -> int:
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x & 0x80000000 else x


class Gpu:
    """tests/_sweep.py os_run's dev on the current device: the members'
    workspaces back to back in one buffer kept across cases, filled and
    checked on the device; only the expected windows are downloaded."""

    def __init__(self):
        self.pool = torch.empty(0, dtype=torch.uint8, device="cuda")
        self.spare = torch.empty(0, dtype=torch.uint8, device="cuda")
        self.status = torch.full((1,), -1, dtype=torch.int64).pin_memory()
        self.word = torch.zeros(1, dtype=torch.int64).pin_memory()
        self.ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.stream = torch.cuda.current_stream()

    def load(self, c):
        self.t = torch.from_numpy(c.arena).cuda()
        assert self.t.data_ptr() % 16 == 0
        need = c.n * c.ws_bytes
        if self.pool.numel() < need:
            self.pool = torch.empty(need, dtype=torch.uint8, device="cuda")
            self.spare = torch.empty(need, dtype=torch.uint8, device="cuda")
        assert self.pool.data_ptr() % 256 == 0 and c.ws_bytes % 256 == 0
        ws = self.ws = self.pool[:need]
        ws.fill_(S.WS_FILL)
        for j in range(c.n if c.ws_bytes else 0):
            m = ws[j * c.ws_bytes:(j + 1) * c.ws_bytes]
            if c.kernel == S.FLAG:
                lo = c.flag_at(0, 0)
                m[lo:lo + 4 * S.SIG_OS_CHUNKS * S.SIG_MAX].view(torch.int32).fill_(_i32(c.epoch + 1))
            else:
                lo = c.ll_slot_at(0)
                w = m[lo:lo + S.LL_PARITY].view(torch.int32).view(-1, 2)
                w[:, 0] = _i32(S.LL_JUNK)
                w[:, 1] = _i32(c.flag)
        self.base = self.spare[:need]
        self.base.copy_(ws)
        self.sym = (ctypes.c_void_p * c.n)(*[ws.data_ptr() + j * c.ws_bytes for j in range(c.n)])
        self.status.fill_(-1)

    def launch(self, c, r, done_val):
        res = c.results[r]
        a = coll.OneShot(
            self.t.data_ptr() + c.sends[r][0], self.t.data_ptr() + res[0] if res else None,
            c.count, c.mode, ctypes.cast(self.sym, ctypes.c_void_p) if c.ws_bytes else None,
            c.slot_bytes, c.parity_off, c.flag_off, c.n, r, c.epoch,
            self.status.data_ptr(), 1, S.OS_TIMEOUT_US,
            self.ctr.data_ptr() if done_val else None,
            self.word.data_ptr() if done_val else None, done_val)
        coll.oneshot_reduce_as(c.op, c.dt, a, self.stream, c.ll)
        self.stream.synchronize()
        status = int(self.status.item()) & S.SIG_NONE
        if not done_val:
            return status, None, None
        return status, int(self.word.item()) & S.SIG_NONE, int(self.ctr.item())

    def gather(self, ranges):
        if not ranges:
            return np.zeros(0, np.uint8)
        return torch.cat([self.ws[lo:lo + nb] for lo, nb in ranges]).cpu().numpy()

    def untouched(self, ranges):
        d = self.ws != self.base
        for lo, nb in ranges:
            d[lo:lo + nb] = False
        return not bool(d.any())

    def refill(self, c):
        for seg in c.results:
            if seg is not None:
                self.t[seg[0]:seg[0] + seg[1]] = S.OUT_FILL

    def arena(self):
        return self.t.cpu().numpy()


@pytest.fixture(scope="module")
def gpu():
    return Gpu()


def test_case_lists_come_to_the_literals():
    """The cases below, from the pair lists: 2455, over all 931 (pair, kernel,
    NLEAF) instantiations (tests/test_sweep_cpu.py holds what each covers)."""
    assert len(S.reduce_pairs()) == 133
    assert sum(S.N_OS_PAIR_CASES * len(S.dts_of(op)) + S.N_OS_OP_CASES for op in OPS) \
        == S.N_OS_CASES == N_CASES == 2455
    assert S.N_OS_INSTANCES == 133 * 7 == 931


@pytest.mark.parametrize("op", OPS)
def test_oneshot_every_pair(op, gpu):
    """Every type of the op through both kernels: the flagged one at 1, 2, 3,
    5 and 8 ranks (NLEAF 1, 2, 2, 4, 8), scattered at 3 and 8, reduced to root
    1 of 2 and root 3 of 5 (the others pass no result); the LL one at 2, 3, 5
    and 8 ranks, scattered at 3 and 8.  Three workgroups, the last partial with
    a tail below 16 bytes; the alignment path and the epoch's parity rotate."""
    ran, seen = 0, set()
    for dt in S.dts_of(op):
        for case in S.os_pair_cases(op, dt, np.random.default_rng(25000 + 32 * op + dt)):
            S.os_run(case, gpu)
            seen.add((dt, case.kernel, case.nleaf))
            ran += 1
    assert ran == 15 * len(S.dts_of(op)) and ran
    assert len(seen) == 7 * len(S.dts_of(op))


@pytest.mark.parametrize("op", OPS)
def test_oneshot_folding_epochs_edges_and_completion(op, gpu):
    """One type of the op each: 4, 6 and 7 ranks (tree_leaves' folding);
    epochs 1, 2, 0x7fffffff and 0xffffffff per (kernel, NLEAF) (both parities,
    the wait's signed compare, the LL flag 2·epoch + 1 wrapping); one element;
    a scatter of n - 1 elements (empty blocks, a NULL result); the LL kernel
    at exactly LFA_OS_LL_BYTES and the flagged one an element above; a part of
    128·4096 + 4096 + 48 bytes (chunk 4144 > 4096, 128 workgroups) at 2 and 3
    ranks; the completion word at 1 and 3 workgroups (done_val in the pinned
    word after every launch, the counter back at 0, reused by the next)."""
    cases = list(S.os_op_cases(op, np.random.default_rng(26000 + op)))
    for case in cases:
        S.os_run(case, gpu)
    assert len(cases) == 46
    assert sum(c.done for c in cases) == 4 and {c.epoch for c in cases} >= set(S.OS_EPOCHS)


def test_entry_own_choice_and_validation(gpu):
    """lfa__oneshot_as with ll = -1 gives a correct result through whichever
    kernel the launcher chooses; it refuses what lfa_oneshot_reduce_async
    refuses, and ll = 1 where the launcher never takes the LL kernel."""
    import os
    rng = np.random.default_rng(6)
    count = S.os_count(S.LL, S.OS_ALL, 3, 4)
    own = S.LL if os.environ.get("LFA_OS_LL", "")[:1] == "1" else S.FLAG
    S.os_run(S.OsCase(S.SUM, 8, 3, S.OS_ALL, count, own, "vec", 1,
                      S.inputs(S.SUM, 8, 3, count, rng), ll=-1), gpu)
    case = S.OsCase(S.SUM, 8, 3, 1, count, S.FLAG, "vec", 1, S.inputs(S.SUM, 8, 3, count, rng))
    gpu.load(case)
    a = coll.OneShot(gpu.t.data_ptr() + case.sends[0][0], None, count, 1,
                     ctypes.cast(gpu.sym, ctypes.c_void_p), case.slot_bytes, case.parity_off,
                     case.flag_off, 3, 0, 1, gpu.status.data_ptr(), 1, S.OS_TIMEOUT_US)
    with pytest.raises(coll.CollError) as e:      # reduce to a root: never LL
        coll.oneshot_reduce_as(S.SUM, 8, a, gpu.stream, 1)
    assert e.value.rc == -LFA_EINVAL
    a.slot_bytes += 16
    for ll in (-1, 0, 1):
        with pytest.raises(coll.CollError) as e:
            coll.oneshot_reduce_as(S.SUM, 8, a, gpu.stream, ll)
        assert e.value.rc == -LFA_EINVAL
        with pytest.raises(coll.CollError) as e:
            coll.oneshot_reduce_as(S.WRITE, 8, a, gpu.stream, ll)
        assert e.value.rc == -LFA_EOPNOTSUPP
    with pytest.raises(coll.CollError) as e:
        coll.oneshot_reduce(S.SUM, 8, a, gpu.stream)
    assert e.value.rc == -LFA_EINVAL
    gpu.stream.synchronize()
    assert gpu.untouched([]) and int(gpu.status.item()) == -1      # nothing was launched
