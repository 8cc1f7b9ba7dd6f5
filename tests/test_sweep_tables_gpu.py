"""Oracle sweep of the three binary tables' own kernels: every write (148),
fetch (145) and compare (84) instantiation in liblfa.so against the reference
(oracle.write / oracle.readwrite / oracle.swap, tests/_half_ref.py for the
half types).

tests/test_sweep_gpu.py covers the tree, tree-put and list forms; this file
the entry points that replace ofi_atomic_write_handlers,
ofi_atomic_readwrite_handlers and ofi_atomic_swap_handlers:
lfa_atomic_write_async (launch_write: combine_lds, combine_elem,
combine_unaligned), lfa_atomic_readwrite_async and lfa_atomic_swap_async
(launch_fetch: fetch_lds drained for the two-input fetch and undrained for the
three-input compare, the guarded register path of a partial tile, fetch_elem
with the ALIGNED and with the byte-wise functor).  Every pair runs on every
path its element size has (tests/_sweep.py, table_layout): all operands
aligned, all one element past a boundary, one operand an element further on,
one operand a byte off, the odd operand rotating so that over an op each of
dst, src, cmp and res takes the odd offset.  One ~40 KiB shape: two whole LDS
tiles, a partial tile with whole and partial waves, a ragged tail.

The compare inputs put "equal", "below" and "above" on a third of the lanes
each, src never equals dst, and the last 64 lanes hold the +-0, NaN, infinity
and type-extreme pairs (swap_inputs); the fetch inputs change dst on at least
a quarter of the lanes (tests/test_sweep_cpu.py holds both to that without a
GPU and runs this case list through the host forms).  Every case is one arena:
afterwards the sentinels between the operands are intact, src and cmp are
unchanged, res is the old dst byte for byte, and dst is the reference's: byte
for byte for the compare table and ATOMIC_READ, through tests/_cmp.py's
assert_parity for what a fetch computes.

Each test counts the cases it ran against the product of its lists, so a
pair that was skipped fails the test.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from libfabric_amd import atomic
from tests import _sweep as S

pytestmark = pytest.mark.gpu

FETCH_ATOMIC, COMPARE_ATOMIC = 1 << 58, 1 << 59       # include/lfa_fabric.h


@pytest.fixture(scope="module")
def manifest(golden_dir):
    with open(os.path.join(golden_dir, "manifest.json")) as f:
        return json.load(f)


def _upload(arena: np.ndarray) -> torch.Tensor:
    t = torch.from_numpy(arena).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _n_cases(dts) -> int:
    return sum(S.N_PATHS[S.esz_of(dt)] for dt in dts)


def test_pair_lists_match_the_library(manifest):
    rp, sp, wp = S.rw_pairs(), S.swap_pairs(), S.write_pairs(manifest)
    assert len(wp) == S.N_WRITE_PAIRS == 148
    assert len(rp) == S.N_RW_PAIRS == 145 and len(sp) == S.N_SWAP_PAIRS == 84
    assert {(op, dt) for op in S.RW_OPS for dt in range(16)
            if atomic.atomic_valid(dt, op, FETCH_ATOMIC) == 0} == set(rp)
    assert {(op, dt) for op in S.SWAP_OPS for dt in range(16)
            if atomic.atomic_valid(dt, op, COMPARE_ATOMIC) == 0} == set(sp)
    assert sum(len(S.table_dts(wp, op)) for op in S.WRITE_OPS) == 148
    assert sum(len(S.table_dts(rp, op)) for op in S.RW_OPS) == 145
    assert sum(len(S.table_dts(sp, op)) for op in S.SWAP_OPS) == 84


@pytest.mark.parametrize("op", S.WRITE_OPS)
def test_write_every_pair(op, manifest):
    """lfa_atomic_write_async: every type of the op, half types included, on
    the vector, head, element and bytes paths."""
    dts = S.table_dts(S.write_pairs(manifest), op)
    cases = list(S.write_cases(op, dts, np.random.default_rng(7000 + op)))
    for dt, case in cases:
        assert atomic.reduce_valid(dt, op) == 0
        t = _upload(case.arena)
        atomic.write(op, dt, case.view(t, "dst"), case.view(t, "src"), S.lanes(S.esz_of(dt)))
        case.check(dt, t.cpu().numpy())
    assert len(cases) == _n_cases(dts) and dts
    S.assert_every_operand_was_odd("write", op, cases)


@pytest.mark.parametrize("op", S.RW_OPS)
def test_readwrite_every_pair(op):
    """lfa_atomic_readwrite_async on every path; ATOMIC_READ with src=None."""
    dts = S.table_dts(S.rw_pairs(), op)
    cases = list(S.readwrite_cases(op, dts, np.random.default_rng(8000 + op)))
    for dt, case in cases:
        t = _upload(case.arena)
        atomic.readwrite(op, dt, case.view(t, "dst"),
                         case.view(t, "src") if "src" in case.at else None,
                         case.view(t, "res"), S.lanes(S.esz_of(dt)))
        case.check(dt, t.cpu().numpy())
    assert len(cases) == _n_cases(dts) and dts
    S.assert_every_operand_was_odd("readwrite", op, cases)


@pytest.mark.parametrize("op", S.SWAP_OPS)
def test_swap_every_pair(op):
    """lfa_atomic_swap_async on every path."""
    dts = S.table_dts(S.swap_pairs(), op)
    cases = list(S.swap_cases(op, dts, np.random.default_rng(9000 + op)))
    for dt, case in cases:
        t = _upload(case.arena)
        atomic.swap(op, dt, case.view(t, "dst"), case.view(t, "src"), case.view(t, "cmp"),
                    case.view(t, "res"), S.lanes(S.esz_of(dt)))
        case.check(dt, t.cpu().numpy())
    assert len(cases) == _n_cases(dts)
    assert len(dts) == {S.CSWAP: 13, S.CSWAP_NE: 13, S.MSWAP: 10}.get(op, 12)
    S.assert_every_operand_was_odd("swap", op, cases)


_RW = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)
_SW = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                       ctypes.c_size_t)


def test_sync_tables_device_pointers():
    """lfa_atomic_readwrite_handlers[op][dt] and lfa_atomic_swap_handlers
    [op - 12][dt], the synchronous entries, with device pointers: every entry
    once on the vec case, held to the same check."""
    L = atomic.lib()
    rw = (ctypes.c_void_p * (12 * 16)).in_dll(L, "lfa_atomic_readwrite_handlers")
    sw = (ctypes.c_void_p * (7 * 16)).in_dll(L, "lfa_atomic_swap_handlers")
    assert L.lfa_atomic_last_error() == 0
    ran = 0
    for op in S.RW_OPS:
        dts = S.table_dts(S.rw_pairs(), op)
        for dt, case in S.readwrite_cases(op, dts, np.random.default_rng(8500 + op), ("vec",)):
            t = _upload(case.arena)
            torch.cuda.synchronize()        # the entry runs on the null stream
            _RW(rw[op * 16 + dt])(case.view(t, "dst").data_ptr(),
                                  case.view(t, "src").data_ptr() if "src" in case.at else None,
                                  case.view(t, "res").data_ptr(), S.lanes(S.esz_of(dt)))
            case.check(dt, t.cpu().numpy())
            ran += 1
    assert ran == 145
    for op in S.SWAP_OPS:
        dts = S.table_dts(S.swap_pairs(), op)
        for dt, case in S.swap_cases(op, dts, np.random.default_rng(9500 + op), ("vec",)):
            t = _upload(case.arena)
            torch.cuda.synchronize()
            _SW(sw[(op - 12) * 16 + dt])(*(case.view(t, k).data_ptr()
                                           for k in ("dst", "src", "cmp", "res")),
                                         S.lanes(S.esz_of(dt)))
            case.check(dt, t.cpu().numpy())
            ran += 1
    assert ran == 145 + 84
    assert L.lfa_atomic_last_error() == 0
